"""Generate tests/golden/g14_backbone.npz and g14_backbone_net.npz by running the REFERENCE's own ResNet classes (build machine only; no test runs this).

Run:  RELATION_DETR_REFERENCE=<checkout of the reference> python tools/gen_golden_backbone.py

Run unmodified from the reference, on the CPU in fp32:
  models/bricks/misc.py                       loaded by file path (it imports only torch): ``FrozenBatchNorm2d``
  models/backbones/resnet.py                  loaded by file path: ``BasicBlock``, ``Bottleneck``, ``ResNet``, ``ResNetBackbone.model_arch``
Stubs -- what resnet.py imports and this machine's torch lacks, none of it on the path of a fixture value
(tests/golden/g14_backbone.md names them too):
  torchvision.models.feature_extraction       ``create_feature_extractor`` raises: nothing here builds the extractor.  The keys of (c)
                                              are the ``ResNet``'s own minus ``fc.*``, which is what the extractor's dead-code
                                              elimination leaves when ``layer4`` is returned (``avgpool`` has no state)
  models.backbones.base_backbone              ``BaseBackbone``: an empty class (the real one needs omegaconf)
  models.bricks.deform_conv2d_pack            ``DeformConv2dPack``: a class that raises when built; no stage here has DCN
  util.lazy_load                              ``LazyCall(cls)(**kw)`` returns ``dict(_target_=cls, **kw)``: the architecture table is read
                                              as data (block, layers, groups, width_per_group), ``instantiate`` raises
  util.tune_mode_convbn, util.utils           the two names resnet.py imports, raising when called

The fixture holds data only.  Keys:
  blk.<name>.sd.<key>         (a) the block's state dict; .x input, .y output, .gy the seeded output gradient, .gx autograd's input
                              gradient, .gw.<parameter> its weight gradients; .cfg = inplanes, planes, stride, groups, base_width,
                              dilation, has_downsample.  Blocks: bneck_s2 (stride 2 + downsample), bneck_g2 (groups = 2), bneck_d2
                              (dilation 2), basic_s2 (BasicBlock, stride 2 + downsample), basic (BasicBlock, identity shortcut)
  net.sd.<key>                (b), in g14_backbone_net.npz: ResNet(Bottleneck, (1, 1, 1, 1), width_per_group=8,
                              norm_layer=FrozenBatchNorm2d): the state dict of the stem, layer1 and layer2, the convolution weights
                              drawn on the fp16 grid and stored as float16 (exact; layer2's 256 -> 512 shortcut alone is 131 k values);
                              net.x the [2, 3, 36, 60] batch; net.stem (behind the max-pool), net.layer1, net.layer2 the outputs
  keys.<arch>.names/.shapes   (c) names (one string, newline separated) and shapes ([n, 4] int64, padded with 0) of the state dict of
                              resnet50 / resnet18 as the reference's classes define them; keys.<arch>.num_channels for
                              return_indices = (1, 2, 3)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g14_backbone.npz")               # (a) and (c)
OUT_NET = os.path.join(ROOT, "tests", "golden", "g14_backbone_net.npz")       # (b): a file of its own, each stays below 1 MiB
# name: (class, inplanes, planes, stride, groups, base_width, dilation, downsample, input H x W)
BLOCKS = {
    "bneck_s2": ("Bottleneck", 32, 16, 2, 1, 64, 1, True, (9, 11)),
    "bneck_g2": ("Bottleneck", 64, 16, 1, 2, 64, 1, False, (5, 7)),
    "bneck_d2": ("Bottleneck", 64, 16, 1, 1, 64, 2, False, (6, 7)),
    "basic_s2": ("BasicBlock", 24, 32, 2, 1, 64, 1, True, (7, 10)),
    "basic": ("BasicBlock", 32, 32, 1, 1, 64, 1, False, (5, 6)),
}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def _raises(what):
    def fn(*args, **kwargs):
        raise RuntimeError(f"{what} is a stub of tools/gen_golden_backbone.py")
    return fn


def import_reference():
    ref = os.environ.get("RELATION_DETR_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "models")):
        sys.exit("set RELATION_DETR_REFERENCE to a checkout of the reference")
    misc = _load("models.bricks.misc", os.path.join(ref, "models", "bricks", "misc.py"))

    def module(name, **names):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(names)
        sys.modules[name] = m
        return m

    if "torchvision" not in sys.modules:
        module("torchvision")
        module("torchvision.models")
    module("torchvision.models.feature_extraction", create_feature_extractor=_raises("create_feature_extractor"))
    module("models")
    module("models.backbones")
    module("models.backbones.base_backbone", BaseBackbone=type("BaseBackbone", (), {}))
    module("models.bricks", misc=misc)
    module("models.bricks.deform_conv2d_pack", DeformConv2dPack=type("DeformConv2dPack", (), {"__init__": _raises("DeformConv2dPack")}))
    module("util")
    module("util.lazy_load", LazyCall=lambda cls: (lambda **kw: dict(_target_=cls, **kw)), instantiate=_raises("instantiate"))
    module("util.tune_mode_convbn", turn_on_efficient_conv_bn_eval_for_single_model=_raises("the conv-bn tuner"))
    module("util.utils", load_checkpoint=_raises("load_checkpoint"))
    return _load("_reference_resnet", os.path.join(ref, "models", "backbones", "resnet.py")), misc


def randomise(module, g):
    """Random convolution weights at the initialisation's scale and random frozen statistics, in place."""
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=g) * 1.5 + 0.25)
            elif name.endswith("running_mean"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.3)
            elif name.endswith("bias"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.2)
            elif t.dim() == 1:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            else:
                fan = t[0].numel()
                t.copy_(torch.randn(t.shape, generator=g) * (1.5 / fan) ** 0.5)


def block_case(resnet, misc, name, seed):
    cls, inplanes, planes, stride, groups, base_width, dilation, down, (h, w) = BLOCKS[name]
    block_cls = getattr(resnet, cls)
    norm = misc.FrozenBatchNorm2d
    downsample = None
    if down:
        downsample = torch.nn.Sequential(resnet.conv1x1(inplanes, planes * block_cls.expansion, stride), norm(planes * block_cls.expansion))
    block = block_cls(inplanes, planes, stride, downsample, groups, base_width, dilation, norm)
    g = torch.Generator().manual_seed(seed)
    randomise(block, g)
    x = torch.randn(2, inplanes, h, w, generator=g).requires_grad_()
    y = block(x)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    data = {"x": x.detach().numpy(), "y": y.detach().numpy(), "gy": gy.numpy(), "gx": x.grad.numpy(),
            "cfg": np.array([inplanes, planes, stride, groups, base_width, dilation, int(down)], dtype=np.int64)}
    data.update({f"sd.{k}": v.numpy() for k, v in block.state_dict().items()})
    data.update({f"gw.{k}": p.grad.numpy() for k, p in block.named_parameters()})
    return data


def net_case(resnet, misc):
    net = resnet.ResNet(resnet.Bottleneck, (1, 1, 1, 1), width_per_group=8, norm_layer=misc.FrozenBatchNorm2d)
    net.eval()                                   # the reference's train() returns None: no chaining
    g = torch.Generator().manual_seed(77)
    randomise(net, g)
    with torch.no_grad():
        for t in net.state_dict().values():      # convolution weights on the fp16 grid: stored as float16, exactly
            if t.dim() == 4:
                t.copy_(t.half().float())
    x = torch.randn(2, 3, 36, 60, generator=g)
    with torch.no_grad():
        stem = net.maxpool(net.relu(net.bn1(net.conv1(x))))
        layer1 = net.layer1(stem)
        layer2 = net.layer2(layer1)
    data = {"x": x.numpy(), "stem": stem.numpy(), "layer1": layer1.numpy(), "layer2": layer2.numpy()}
    data.update({f"sd.{k}": (v.half() if v.dim() == 4 else v).numpy() for k, v in net.state_dict().items()
                 if k.split(".")[0] in ("conv1", "bn1", "layer1", "layer2")})
    return data


def key_table(resnet, misc, arch):
    cfg = resnet.ResNetBackbone.model_arch[arch]
    kwargs = {k: v for k, v in cfg.items() if k not in ("_target_", "url")}
    net = cfg["_target_"](norm_layer=misc.FrozenBatchNorm2d, **kwargs)
    sd = {k: v for k, v in net.state_dict().items() if not k.startswith("fc.")}
    shapes = np.zeros((len(sd), 4), dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    return {"names": np.array("\n".join(sd)), "shapes": shapes,
            "num_channels": np.array([64 * kwargs["block"].expansion * 2 ** i for i in (1, 2, 3)], dtype=np.int64)}


def main():
    resnet, misc = import_reference()
    out = {}
    for seed, name in enumerate(BLOCKS):
        data = block_case(resnet, misc, name, 100 + seed)
        out.update({f"blk.{name}.{k}": v for k, v in data.items()})
        print(name, "x", data["x"].shape, "y", data["y"].shape, "max |y|", float(np.abs(data["y"]).max()))
    data = net_case(resnet, misc)
    np.savez_compressed(OUT_NET, **{f"net.{k}": v for k, v in data.items()})
    print(f"wrote {OUT_NET}: {os.path.getsize(OUT_NET)} bytes")
    print("net", {k: data[k].shape for k in ("x", "stem", "layer1", "layer2")})
    for arch in ("resnet50", "resnet18"):
        data = key_table(resnet, misc, arch)
        out.update({f"keys.{arch}.{k}": v for k, v in data.items()})
        print(arch, len(data["shapes"]), "keys", data["num_channels"].tolist())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
