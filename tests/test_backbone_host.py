"""CPU side of the ResNet backbone (relation_detr_amd/backbones): the torch route against the reference's own classes
(tests/golden/g14_backbone*.npz, tools/gen_golden_backbone.py), the state-dict contract, loading, freezing, refusals, and the
C ABI's validation, which precedes every HIP call and so runs without a GPU."""
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
from relation_detr_amd import _lib, backbones, detector, options
from relation_detr_amd.backbones import BasicBlock, Bottleneck, FrozenBatchNorm2d, ResNet, ResNetBackbone
from relation_detr_amd.backbones import resnet as resnet_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = ("bneck_s2", "bneck_g2", "bneck_d2", "basic_s2", "basic")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float() if a.dtype.kind == "f" else torch.from_numpy(np.ascontiguousarray(a))


def ulps_of_max(got: np.ndarray, ref: np.ndarray) -> float:
    """max |got - ref| in units of the fp32 spacing at the reference's largest magnitude (tests/test_neck_host.py)."""
    return float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / np.spacing(np.float32(np.abs(ref).max())))


@pytest.fixture(scope="module")
def g14():
    z = load_golden("g14_backbone.npz")
    z.update(load_golden("g14_backbone_net.npz"))
    return z


def golden_block(g14, name):
    inplanes, planes, stride, groups, base_width, dilation, down = g14[f"blk.{name}.cfg"].tolist()
    cls = Bottleneck if name.startswith("bneck") else BasicBlock
    downsample = None
    if down:
        downsample = nn.Sequential(resnet_mod.conv1x1(inplanes, planes * cls.expansion, stride), FrozenBatchNorm2d(planes * cls.expansion))
    block = cls(inplanes, planes, stride, downsample, groups, base_width, dilation, FrozenBatchNorm2d)
    prefix = f"blk.{name}.sd."
    block.load_state_dict({k[len(prefix):]: T(v) for k, v in g14.items() if k.startswith(prefix)}, strict=True)
    return block


# ----------------------------------------------------------------------------------------------- the torch route against g14
def test_blocks_torch_route_match_the_reference_forward_and_backward(g14):
    worst = 0.0
    for name in BLOCKS:
        block = golden_block(g14, name)
        x = T(g14[f"blk.{name}.x"]).requires_grad_()
        y = block.forward_torch(x)
        y.backward(T(g14[f"blk.{name}.gy"]))
        worst = max(worst, ulps_of_max(y.detach().numpy(), g14[f"blk.{name}.y"]), ulps_of_max(x.grad.numpy(), g14[f"blk.{name}.gx"]))
        params = dict(block.named_parameters())
        stored = [k for k in g14 if k.startswith(f"blk.{name}.gw.")]
        assert sorted(k.rsplit(".gw.", 1)[1] for k in stored) == sorted(params), name
        for k in stored:
            worst = max(worst, ulps_of_max(params[k.rsplit(".gw.", 1)[1]].grad.numpy(), g14[k]))
    print(f"blocks, torch route vs reference: worst {worst:.2f} ulp of the tensor's maximum")
    assert worst <= 4.0, worst


def test_network_torch_route_matches_the_reference(g14):
    net = ResNet(Bottleneck, (1, 1, 1, 1), width_per_group=8, norm_layer=FrozenBatchNorm2d, stages=2, head=False).eval()
    net.load_state_dict({k[len("net.sd."):]: T(v) for k, v in g14.items() if k.startswith("net.sd.")}, strict=True)
    x = T(g14["net.x"])
    with torch.no_grad():
        stem = net.maxpool(net.relu(net.bn1(net.conv1(x))))
        layer1, layer2 = net.stages_torch(x)
        assert all(torch.equal(a, b) for a, b in zip(net(x), (layer1, layer2)))        # CPU tensors take the torch route
    worst = max(ulps_of_max(stem.numpy(), g14["net.stem"]), ulps_of_max(layer1.numpy(), g14["net.layer1"]),
                ulps_of_max(layer2.numpy(), g14["net.layer2"]))
    print(f"network, torch route vs reference: worst {worst:.2f} ulp of the tensor's maximum")
    assert worst <= 4.0, worst


def test_frozen_norm_is_the_reference_expression():
    g = torch.Generator().manual_seed(3)
    norm = FrozenBatchNorm2d(7, eps=1e-3)
    assert list(norm.state_dict()) == ["weight", "bias", "running_mean", "running_var"] and not list(norm.parameters())
    sd = {"weight": torch.rand(7, generator=g) + 0.5, "bias": torch.randn(7, generator=g), "running_mean": torch.randn(7, generator=g),
          "running_var": torch.rand(7, generator=g) + 0.1, "num_batches_tracked": torch.tensor(5)}
    norm.load_state_dict(sd, strict=True)
    x = torch.randn(2, 7, 3, 5, generator=g)
    scale = sd["weight"] * (sd["running_var"] + 1e-3).rsqrt()
    shift = sd["bias"] - sd["running_mean"] * scale
    assert torch.equal(norm(x), x * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1))
    s, h = norm.scale_shift()
    assert s.dtype == torch.float32 and tuple(s.shape) == (7,) and torch.equal(s, scale) and torch.equal(h, shift)
    assert norm.scale_shift()[0] is s                                              # cached ...
    norm.weight.mul_(2.0)                                                          # ... on the buffers' version
    assert torch.equal(norm.scale_shift()[0], 2.0 * sd["weight"] * (sd["running_var"] + 1e-3).rsqrt())
    assert repr(norm) == "FrozenBatchNorm2d(7, eps=0.001)"


# ----------------------------------------------------------------------------------------------- keys, loading, freezing
@pytest.mark.parametrize("arch", ["resnet50", "resnet18"])
def test_state_dict_is_the_reference_feature_extractors(g14, arch):
    model = ResNetBackbone(arch, return_indices=(1, 2, 3))
    names = str(g14[f"keys.{arch}.names"]).split("\n")
    shapes = [tuple(int(d) for d in row if d) for row in g14[f"keys.{arch}.shapes"]]
    sd = model.state_dict()
    assert list(sd) == names
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert model.num_channels == g14[f"keys.{arch}.num_channels"].tolist()
    assert model.return_layers == ["layer2", "layer3", "layer4"]
    assert not hasattr(model, "fc") and not hasattr(model, "avgpool")


def test_only_the_returned_stages_are_built():
    model = ResNetBackbone("resnet50", return_indices=(0, 1))
    assert not [k for k in model.state_dict() if k.startswith(("layer3.", "layer4."))]
    assert model.num_channels == [256, 512] and model.return_layers == ["layer1", "layer2"]
    out = model(torch.zeros(1, 3, 33, 47))
    assert list(out) == ["layer1", "layer2"] and tuple(out["layer2"].shape) == (1, 512, 5, 6)
    with pytest.raises(ValueError):
        ResNetBackbone("resnet50", return_indices=(0, 1), freeze_indices=(3,))
    with pytest.raises(ValueError):
        ResNetBackbone("resnet51")


def full_checkpoint(arch="resnet18"):
    """A state dict as torchvision's full classifier writes it: every stage, ``fc.*`` and ``num_batches_tracked``."""
    block, layers, groups, width = backbones.ARCHITECTURES[arch]
    full = ResNet(block, layers, groups=groups, width_per_group=width, norm_layer=nn.BatchNorm2d)
    g = torch.Generator().manual_seed(5)
    sd = {k: (torch.randn(v.shape, generator=g) * 0.1 if v.dtype.is_floating_point else v.clone()) for k, v in full.state_dict().items()}
    sd.update({k: v.abs() + 0.5 for k, v in sd.items() if k.endswith("running_var")})
    assert "fc.weight" in sd and "bn1.num_batches_tracked" in sd and "layer4.1.bn2.num_batches_tracked" in sd
    return sd


def test_a_full_checkpoint_loads_strictly(tmp_path):
    sd = full_checkpoint()
    for kwargs in (dict(return_indices=(1, 2, 3)), dict(return_indices=(0, 1))):
        model = ResNetBackbone("resnet18", **kwargs)
        model.load_state_dict(dict(sd), strict=True)
        built = ResNetBackbone("resnet18", weights={"model": dict(sd)}, **kwargs)
        for k, v in model.state_dict().items():
            assert torch.equal(v, sd[k]) and torch.equal(built.state_dict()[k], sd[k]), k
    path = tmp_path / "resnet18.pth"
    torch.save(sd, path)
    from_path = ResNetBackbone("resnet18", weights=str(path), return_indices=(3,))
    assert torch.equal(from_path.layer4[1].conv2.weight, sd["layer4.1.conv2.weight"])
    with pytest.raises(RuntimeError):                                              # strict: a missing key is an error
        ResNetBackbone("resnet18").load_state_dict({k: v for k, v in sd.items() if k != "conv1.weight"})
    wrapped = nn.Module()                                                          # as the detector holds it: the reference's backbone.* keys
    wrapped.backbone = ResNetBackbone("resnet18", return_indices=(1, 2, 3), freeze_indices=(0,))
    wrapped.load_state_dict({f"backbone.{k}": v for k, v in sd.items()}, strict=True)


def test_freezing_follows_the_reference_and_norms_stay_in_eval_mode():
    model = ResNetBackbone("resnet50", return_indices=(1, 2, 3), freeze_indices=(0,))
    for name, p in model.named_parameters():
        frozen = name.split(".")[0] in ("conv1", "layer1")
        assert p.requires_grad == (not frozen), name
    assert all(p.requires_grad for p in ResNetBackbone("resnet18", freeze_indices=()).parameters())
    only_stem_and_3 = ResNetBackbone("resnet18", freeze_indices=(2,))
    assert {n.split(".")[0] for n, p in only_stem_and_3.named_parameters() if not p.requires_grad} == {"conv1", "layer3"}
    model.train()
    assert model.training and model.layer2[0].conv1.training
    assert all(not m.training for m in model.modules() if isinstance(m, FrozenBatchNorm2d))
    plain = ResNetBackbone("resnet18", norm_layer=nn.BatchNorm2d).train()
    assert all(not m.training for m in plain.modules() if isinstance(m, nn.BatchNorm2d))
    assert not plain.takes_fused_route(torch.zeros(1, 3, 8, 8))


# ----------------------------------------------------------------------------------------------- refusals
def test_dcn_is_refused():
    with pytest.raises(NotImplementedError):
        ResNetBackbone("resnet50", stage_with_dcn=(False, True, True, True))
    with pytest.raises(NotImplementedError):
        Bottleneck(64, 16, with_dcn=True)
    ResNetBackbone("resnet18", return_indices=(0,), stage_with_dcn=(False,) * 4)


def test_fused_calls_have_no_cpu_path():
    x, s, h = torch.randn(1, 4, 5, 6), torch.ones(4), torch.zeros(4)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):
        backbones.frozen_bn_act(x, s, h)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):
        backbones.frozen_bn_act_backward(x, x, s)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):
        backbones.stem_bn_relu_maxpool(x, s, h)
    model = ResNetBackbone("resnet18", return_indices=(1, 3), freeze_indices=(0,)).eval()          # fused=True
    image = torch.randn(2, 3, 40, 56)
    assert model.fused and not model.takes_fused_route(image)
    with torch.no_grad():
        got, want = model(image), ResNetBackbone.forward_torch(model, image)
    assert list(got) == ["layer2", "layer4"] and all(torch.equal(got[k], want[k]) for k in got)
    assert all(v.is_contiguous() for v in got.values())


# ----------------------------------------------------------------------------------------------- the C ABI without a GPU
ONE, TWO, P8 = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20), ctypes.c_void_p(4096 + 8)
SHAPE = dict(B=1, C=4, H=5, W=6)                                                   # 120 elements: 480 bytes in fp32
INSIDE = ctypes.c_void_p(4096 + 64)                                                # overlaps [4096, 4096 + 480) without being it
HUGE = dict(B=2, C=1024, H=1024, W=1024)                                           # 2^31 elements
BAD_SHAPES = [({"B": 0}, -1), ({"C": -3}, -1), ({"H": 0}, -1), ({"W": -1}, -1), ({"channels_last": 2}, -1)]
FWD = ("x scale shift residual B C H W channels_last relu out stream",
       dict(x=ONE, scale=ONE, shift=ONE, residual=None, channels_last=0, relu=1, out=ONE, stream=None, **SHAPE),
       BAD_SHAPES + [({"x": None}, -1), ({"scale": None}, -1), ({"shift": None}, -1), ({"out": None}, -1), ({"relu": 3}, -1),
                     ({"residual": ONE}, -1), ({"residual": INSIDE}, -1), ({"out": INSIDE}, -1), (HUGE, -2), (dict(HUGE, channels_last=1), -2),
                     ({"x": P8, "out": P8}, -2), ({"scale": P8}, -2), ({"residual": P8, "x": TWO, "out": TWO}, -2)])
BWD = ("dy y scale B C H W channels_last relu dx dres stream",
       dict(dy=ONE, y=TWO, scale=ONE, channels_last=0, relu=1, dx=ONE, dres=None, stream=None, **SHAPE),
       BAD_SHAPES + [({"dy": None}, -1), ({"scale": None}, -1), ({"dx": None}, -1), ({"y": None}, -1), ({"relu": -1}, -1),
                     ({"dres": ONE}, -1), ({"dres": INSIDE}, -1), ({"y": ONE}, -1), ({"dx": INSIDE}, -1), (HUGE, -2),
                     ({"dy": P8, "dx": P8}, -2), ({"y": None, "relu": 0, "dx": P8, "dy": P8}, -2)])
POOL = ("x scale shift B C H W channels_last out stream",
        dict(x=ONE, scale=ONE, shift=ONE, channels_last=0, out=TWO, stream=None, **SHAPE),
        BAD_SHAPES + [({"x": None}, -1), ({"scale": None}, -1), ({"shift": None}, -1), ({"out": None}, -1), ({"out": ONE}, -1),
                      ({"out": INSIDE}, -1), (HUGE, -2), ({"x": P8}, -2), ({"shift": P8}, -2)])
TABLE = {f"rdetr_frozen_bn_act_{t}": FWD for t in ("f32", "bf16")}
TABLE.update({f"rdetr_frozen_bn_act_backward_{t}": BWD for t in ("f32", "bf16")})
TABLE.update({f"rdetr_stem_pool_{t}": POOL for t in ("f32", "bf16")})


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
    lib = _lib.load()
    for name in TABLE:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(re.findall(rf"^int {name}\s*\(", header, re.M)) == 1, name
        declared = re.search(rf"^int {name}\s*\(([^;]*)\);", header, re.M | re.S).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name]) == len(TABLE[name][0].split()), name
        assert not name.startswith("rdetr_image_")
    assert "#define RDETR_ABI_VERSION 3" in header and lib.rdetr_abi_version() == 3
    assert "backbone.hip" in open(os.path.join(ROOT, "relation_detr_amd", "csrc", "Makefile")).read()
    assert len(dataclasses.fields(options.Options)) == 25                        # `fused` is a constructor argument
    for name in ("ResNetBackbone", "ResNet", "FrozenBatchNorm2d"):
        assert name in relation_detr_amd.__all__ and getattr(relation_detr_amd, name) is getattr(backbones, name)
    assert relation_detr_amd.relation_detr_r50 is detector.relation_detr_r50


def test_r50_detector_has_the_reference_layout():
    model = relation_detr_amd.relation_detr_r50(num_classes=11, num_queries=30, hybrid_num_proposals=30, enc_layers=1, dec_layers=1, d_ffn=32)
    assert isinstance(model.backbone, ResNetBackbone) and model.backbone.arch == "resnet50"
    assert model.backbone.return_layers == ["layer2", "layer3", "layer4"] and model.backbone.freeze_indices == (0,)
    assert [c[0].in_channels for c in model.neck.convs][:3] == [512, 1024, 2048] and len(model.neck.convs) == 4
    keys = [k for k in model.state_dict() if k.startswith("backbone.")]
    assert keys == [f"backbone.{k}" for k in model.backbone.state_dict()] and "backbone.layer4.2.bn3.running_var" in keys
    assert model.preprocessor.resize == (800, 1333) and model.num_select == 300
