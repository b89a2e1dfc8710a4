"""Host side of the neck and the position encoding (relation_detr_amd/neck.py, RelationDETR): the torch route against the reference's
recorded results (tests/golden/g12_neck.npz), the state-dict contract, the input rules, the ABI, the parameter groups and one
train_step on the CPU.  Needs no GPU."""
import dataclasses
import os
import re
from functools import partial

import numpy as np
import pytest
import torch
from torch import nn

import relation_detr_amd
from conftest import load_golden
from helpers import synthetic_state_dict
from relation_detr_amd import _lib, detector, neck, options
from relation_detr_amd.neck import ChannelMapper, PositionEmbeddingSine, PyramidBuilder
from relation_detr_amd.optim import FusedAdamW, relation_param_groups, train_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
SYMBOLS = ("rdetr_neck_workspace_bytes", "rdetr_group_norm_levels_f32", "rdetr_group_norm_levels_bf16",
           "rdetr_group_norm_levels_backward_f32", "rdetr_group_norm_levels_backward_bf16", "rdetr_pyramid_masks",
           "rdetr_pyramid_sine_pos_f32", "rdetr_pyramid_sine_pos_bf16")
EXPORTS = ("ChannelMapper", "PositionEmbeddingSine", "PyramidBuilder", "GroupNormLevelsFunction", "group_norm_levels", "pyramid_masks",
           "pyramid_sine_pos")
IN_CHANNELS, SIZES = (16, 24, 40), ((12, 20), (6, 10), (3, 5), (2, 3))
POS_TOL = 5e-6                   # the project's bound for sine features of arguments up to 2 pi (tests/shadow.py, sine_pos_embed)


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_neck.npz")


def golden_mapper(z, num_outs=4, prefix="sd.", fused=False):
    m = ChannelMapper(list(IN_CHANNELS), 32, num_outs, norm_layer=partial(nn.GroupNorm, 8), fused=fused)
    m.load_state_dict({k[len(prefix):]: T(v) for k, v in z.items() if k.startswith(prefix)})
    return m


def ulps_of_max(got: np.ndarray, ref: np.ndarray) -> float:
    """max |got - ref| in units of the fp32 spacing at the reference's largest magnitude."""
    return float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / np.spacing(np.float32(np.abs(ref).max())))


def pos_ok_pixels(mask: np.ndarray) -> np.ndarray:
    """[B, h, w]: the pixel's row and its column both hold a valid pixel, i.e. neither normaliser ``last`` is 0."""
    valid = ~mask
    return valid.any(1, keepdims=True) & valid.any(2, keepdims=True)


def test_channel_mapper_torch_route_matches_the_reference(g12):
    m = golden_mapper(g12)
    xs = [T(g12[f"x{i}"]).clone().requires_grad_() for i in range(3)]
    ys = m({str(i): x for i, x in enumerate(xs)})
    assert [tuple(y.shape[-2:]) for y in ys] == list(SIZES)
    sum((y * T(g12[f"go{i}"])).sum() for i, y in enumerate(ys)).backward()
    worst = 0.0
    for i, y in enumerate(ys):
        worst = max(worst, ulps_of_max(y.detach().numpy(), g12[f"y{i}"]))
    for k, p in m.named_parameters():
        worst = max(worst, ulps_of_max(p.grad.numpy(), g12[f"gsd.{k}"]))
    for i, x in enumerate(xs):
        worst = max(worst, ulps_of_max(x.grad.numpy(), g12[f"gx{i}"]))
    print(f"ChannelMapper torch route vs reference: worst {worst:.2f} ulp of the tensor's maximum")
    assert worst <= 4.0, worst
    m5 = golden_mapper(g12, 5, "sd5.")
    with torch.no_grad():
        y5 = m5([T(g12[f"x{i}"]) for i in range(3)])
    assert tuple(y5[4].shape[-2:]) == (1, 2)
    for i, y in enumerate(y5):
        assert ulps_of_max(y.numpy(), g12[f"y5_{i}"]) <= 4.0, i


def test_masks_and_position_encoding_torch_route_match_the_reference(g12):
    pe = PositionEmbeddingSine(16, 10000, True, offset=-0.5)
    pe_u = PositionEmbeddingSine(16, 10000, False, offset=0.0)
    assert list(pe.state_dict()) == [] and pe.dim_t.dtype == torch.float32 and tuple(pe.dim_t.shape) == (8,)
    builder = PyramidBuilder(golden_mapper(g12), pe)
    feats = [T(g12[f"x{i}"]) for i in range(3)]
    with torch.no_grad():
        for img, mk, pk in (("img_mask", "m", "pos"), ("img_mask_rand", "mr", "posr")):
            got_feats, masks, pos = builder(feats, T(g12[img]))
            for i in range(4):
                assert masks[i].dtype == torch.bool and np.array_equal(masks[i].numpy(), g12[f"{mk}{i}"]), (img, i)
                assert pos[i].is_contiguous() and pos[i].dtype == torch.float32 and tuple(pos[i].shape) == (2, 32) + SIZES[i]
                got, ref = pos[i].numpy(), g12[f"{pk}{i}"]
                ok = pos_ok_pixels(g12[f"{mk}{i}"])[:, None]
                assert np.isfinite(got).all()
                assert (np.abs(got - ref) * ok).max() <= POS_TOL, (img, i)
        assert not pos_ok_pixels(g12["mr0"]).all() and not pos_ok_pixels(g12["m0"]).all()      # the exclusion is exercised
        for i in range(4):
            got = pe_u(T(g12[f"m{i}"])).numpy()
            assert np.abs(got - g12[f"posu{i}"]).max() <= POS_TOL, i
    with pytest.raises(ValueError):
        PositionEmbeddingSine(16, (10000, 20, 30))
    pair = PositionEmbeddingSine(16, (10000, 20), True)
    assert tuple(pair(T(g12["m1"])).shape) == (2, 32, 6, 10)


def test_state_dict_keys_are_the_references():
    m = ChannelMapper([512, 1024, 2048], 256, 4)
    want = [f"convs.{i}.{k}" for i in range(4) for k in ("0.weight", "1.weight", "1.bias")]
    assert list(m.state_dict()) == want
    assert m.num_channels == [256] * 4 and m.in_channels == [512, 1024, 2048]
    assert tuple(m.convs[3][0].weight.shape) == (256, 2048, 3, 3) and m.convs[3][0].stride == (2, 2) and m.convs[0][0].bias is None
    assert isinstance(m.convs[0][1], nn.GroupNorm) and m.convs[0][1].num_groups == 32
    plain = ChannelMapper([8], 8, 1, norm_layer=None, activation_layer=nn.ReLU)
    assert list(plain.state_dict()) == ["convs.0.0.weight", "convs.0.0.bias"] and float(plain.convs[0][0].bias.detach().abs().max()) == 0.0

    from test_denoising_host import tiny_head
    head = tiny_head("cpu", False)
    model = detector.RelationDETR(ChannelMapper(list(IN_CHANNELS), 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                                  head.transformer, head.criterion, head.denoising_generator)
    neck_keys = [f"neck.convs.{i}.{k}" for i in range(4) for k in ("0.weight", "1.weight", "1.bias")]
    assert list(model.state_dict()) == neck_keys + list(head.state_dict())
    assert not any(k.startswith("position_embedding") for k in model.state_dict())


def test_input_rules(g12):
    m = golden_mapper(g12)
    xs = [T(g12[f"x{i}"]) for i in range(3)]
    with torch.no_grad():
        from_dict = m({"a": xs[0], "b": xs[1], "c": xs[2]})
        from_list = m(xs)
        assert all(torch.equal(a, b) for a, b in zip(from_dict, from_list))
        last_two = m(xs[1:])                                                     # fewer inputs: the last two convs and the extra level
        assert len(last_two) == 3 and all(torch.equal(a, b) for a, b in zip(last_two, from_list[1:]))
        with pytest.raises(AssertionError):
            m(xs + [xs[2]])
    assert not m.takes_fused_route(xs)                                           # CPU tensors: always the torch route
    assert not ChannelMapper([8], 8, 2, norm_layer=nn.BatchNorm2d).takes_fused_route(xs)
    with pytest.raises(_lib.RdetrError):
        neck.group_norm_levels(xs[:1], [torch.ones(16)], [torch.zeros(16)], 8)   # the kernels have no CPU path


def test_abi_and_exports():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and len(re.findall(rf"\b{name}\s*\(", header)) >= 1, name
    assert len(re.findall(r"^long long rdetr_neck_workspace_bytes\s*\(", header, re.M)) == 1
    assert "#define RDETR_ABI_VERSION 3" in header and _lib.load().rdetr_abi_version() == 3
    assert len(dataclasses.fields(options.Options)) == 25                        # `fused` is a constructor argument here too
    for name in EXPORTS:
        assert name in relation_detr_amd.__all__ and getattr(relation_detr_amd, name) is getattr(neck, name)
    assert "RelationDETR" in relation_detr_amd.__all__ and relation_detr_amd.RelationDETR is detector.RelationDETR
    assert "neck.hip" in open(os.path.join(ROOT, "relation_detr_amd", "csrc", "Makefile")).read()
    import ctypes
    lib = _lib.load()
    hw = (ctypes.c_int * 4)(100, 168, 13, 21)
    # forward: 3 floats per 4096-element chunk of a group; backward: 2 per 4096-pixel chunk of a channel
    fwd = 3 * 4 * (32 * (-(-8 * 16800 // 4096)) + 32 * 1)
    bwd = 2 * 4 * (256 * (-(-16800 // 4096)) + 256 * 1)
    assert lib.rdetr_neck_workspace_bytes(hw, 2, 1, 256, 32) == max(fwd, bwd)
    assert lib.rdetr_neck_workspace_bytes(hw, 2, 1, 256, 8) == -1                # 32 channels per group
    assert lib.rdetr_neck_workspace_bytes(hw, 2, 1, 250, 32) == -1
    assert lib.rdetr_group_norm_levels_f32(None, None, None, hw, 2, 1, 256, 32, 1e-5, None, 0, None, None, None, None) == -1
    assert lib.rdetr_pyramid_masks(None, 0, 1, 8, 8, hw, 2, None, None, None) == -1
    assert lib.rdetr_pyramid_sine_pos_f32(None, hw, 2, 1, 16, None, 1, 6.28, 1e-6, -0.5, None, None) == -1


def test_param_groups_cover_the_neck_and_train_step_moves_it(g12):
    from oracle.cpu_modules import OracleMSDA, OracleRelation, OracleSelfAttention
    from relation_detr_amd import denoising as dn
    from test_denoising_host import EXPECTED_KEYS, C, tiny_head
    head = tiny_head("cpu", False, msda_cls=OracleMSDA, self_attn_cls=OracleSelfAttention, relation_cls=OracleRelation)
    mapper = ChannelMapper(list(IN_CHANNELS), 256, 4, fused=False)
    mapper.load_state_dict(synthetic_state_dict(mapper.state_dict()))
    model = detector.RelationDETR(mapper, PositionEmbeddingSine(128, 10000, True, offset=-0.5, fused=False), head.transformer,
                                  head.criterion, head.denoising_generator).train()
    groups = relation_param_groups(model, 1e-4)
    grouped = [id(p) for g in groups for p in g["params"]]
    assert sorted(grouped) == sorted(id(p) for p in model.parameters()) and len(set(grouped)) == len(grouped)
    default = {id(p) for p in groups[0]["params"]}
    assert "lr" not in groups[0] and "weight_decay" not in groups[0]
    for name, p in model.neck.named_parameters():
        assert (id(p) in default) == (not name.endswith("bias")), name             # the reference sorts by name: convs.{i}.1.weight too
    no_decay = [g for g in groups if g.get("weight_decay") == 0 and "lr" not in g]
    assert len(no_decay) == 1 and all(any(p is q for q in no_decay[0]["params"]) for n, p in model.neck.named_parameters() if n.endswith("bias"))

    z = load_golden("g10_criterion.npz")
    targets = [{"labels": T(z[f"tgt.labels.{b}"]), "boxes": T(z[f"tgt.boxes.{b}"])} for b in range(2)]
    feats = [T(g12[f"x{i}"]) for i in range(3)]
    opt = FusedAdamW(groups, lr=1e-4, weight_decay=1e-4, fused=False)
    before = {k: v.detach().clone() for k, v in model.neck.named_parameters()}
    noise = dn.cdn_noise(11, 2 * dn.denoising_groups(6, 3) * 5, C, "cpu")
    losses, norm = train_step(model, opt, feats, T(g12["img_mask"]), None, targets, max_norm=0.1, noise=noise)
    assert set(losses) == EXPECTED_KEYS and all(torch.isfinite(v) for v in losses.values()) and torch.isfinite(norm)
    for k, p in model.neck.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
        assert not torch.equal(p.detach(), before[k]), k
    model.eval()
    with torch.no_grad():
        logits, boxes = model(feats, T(g12["img_mask"]))
    assert tuple(logits.shape) == (2, 24, C) and tuple(boxes.shape) == (2, 24, 4)
