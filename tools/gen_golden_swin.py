"""Generate tests/golden/g16_swin.npz and g16_swin_net.npz by running the REFERENCE's own Swin classes (build machine only; no test runs this).

Run:  RELATION_DETR_REFERENCE=<checkout of the reference> python tools/gen_golden_swin.py

Run unmodified from the reference, on the CPU, in EVAL mode, in fp32 and once more in float64:
  models/bricks/misc.py                       loaded by file path (it imports only torch): ``MLP``, ``Permute``
  models/backbones/swin.py                    loaded by file path: ``ShiftedWindowAttention`` / ``shifted_window_attention``,
                                              ``SwinTransformer``, ``SwinTransformerBackbone.model_arch``
Stubs -- what swin.py imports and this machine lacks (tests/golden/g16_swin.md names them too):
  omegaconf                                   ``OmegaConf``: an empty class; only ``SwinTransformerBackbone.__new__`` uses it, which nothing here calls
  torchvision.models.feature_extraction       ``create_feature_extractor`` raises: nothing here builds the extractor.  The keys of (c) are
                                              the ``SwinTransformer``'s own minus ``norm.*`` / ``head.*``, which is what the extractor's
                                              dead-code elimination leaves when ``features.7`` is returned
  torchvision.ops                             ``StochasticDepth(p, mode)``: the identity.  Exact in eval mode, the only mode used here
  models.backbones.base_backbone              ``BaseBackbone``: an empty class (the real one needs omegaconf)
  util.lazy_load                              ``LazyCall(cls)(**kw)`` returns ``dict(_target_=cls, **kw)``: the architecture table is read as
                                              data; ``instantiate`` raises
  util.utils                                  ``load_checkpoint`` raises

The fixture holds data only.  Keys of g16_swin.npz:
  att.<case>.cfg                 (a) H, W, wh, ww, sh, sw (the module's shift, before the reference's rule), B, C, heads
  att.<case>.x / .y              input [B, H, W, C] and the fp32 output of ``ShiftedWindowAttention.forward``
  att.<case>.qkv_w/.qkv_b/.proj_w/.proj_b/.table     the module's parameters
  att.<case>.index               its ``relative_position_index`` buffer
  att.<case>.mask                the ``attn_mask`` [windows, N, N] the reference built inside the call ([0] when it built none)
  att.<case>.err                 [max-abs, relative-L2] distance of the fp32 output from the reference run in float64
  keys.<arch>.names/.shapes      (c) names (one string, newline separated) and shapes ([n, 4] int64, padded with 0) of the state dict of
                                 swin_t / swin_l without ``norm.*`` / ``head.*``; keys.<arch>.num_channels for return_indices = (1, 2, 3)
Keys of g16_swin_net.npz (a file of its own: each stays below 1 MiB):
  net.cfg                        (b) embed_dim, depths, heads, window, mlp_ratio of ``SwinTransformer(patch_size=[4, 4], embed_dim=64,
                                 depths=[2, 2], num_heads=[2, 4], window_size=[7, 7], mlp_ratio=2.0)``
  net.sd.<key>                   the state dict of ``features.*``; tensors of two or more dimensions drawn on the fp16 grid and stored
                                 as float16 (exact)
  net.x                          the [2, 3, 36, 68] batch;  net.f1, net.f3 the fp32 outputs of ``features.1`` and ``features.3``
  net.err.f1 / net.err.f3        [max-abs, relative-L2] distance of those from the reference run in float64
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g16_swin.npz")
OUT_NET = os.path.join(ROOT, "tests", "golden", "g16_swin_net.npz")
# name: (window, shift, map, B) -- all with C = 64 and 2 heads
CASES = {
    "w7_s3_9x17": ((7, 7), (3, 3), (9, 17), 2),        # padding on both sides, 6 windows
    "w7_s3_5x17": ((7, 7), (3, 3), (5, 17), 1),        # the row shift is zeroed, the column shift stays
    "w7_s3_5x6": ((7, 7), (3, 3), (5, 6), 1),          # one window, 19 padding tokens, no shift
    "w7_s0_14x7": ((7, 7), (0, 0), (14, 7), 1),        # no shift, no padding
    "w12_s6_13x25": ((12, 12), (6, 6), (13, 25), 1),   # 144 keys: three chunks, the last with 16
    "w3x5_s1x2_7x11": ((3, 5), (1, 2), (7, 11), 1),    # non-square: the 2 * ww - 1 multiplier
}
C, HEADS = 64, 2


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def _raises(what):
    def fn(*args, **kwargs):
        raise RuntimeError(f"{what} is a stub of tools/gen_golden_swin.py")
    return fn


class _Identity(torch.nn.Module):
    def __init__(self, p=0.0, mode="row"):
        super().__init__()
        self.p, self.mode = p, mode

    def forward(self, x):
        return x


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

    module("omegaconf", OmegaConf=type("OmegaConf", (), {}))
    if "torchvision" not in sys.modules:
        module("torchvision")
        module("torchvision.models")
    module("torchvision.models.feature_extraction", create_feature_extractor=_raises("create_feature_extractor"))
    module("torchvision.ops", StochasticDepth=_Identity)
    module("models")
    module("models.backbones")
    module("models.backbones.base_backbone", BaseBackbone=type("BaseBackbone", (), {}))
    module("models.bricks", misc=misc)
    module("util")
    module("util.lazy_load", LazyCall=lambda cls: (lambda **kw: dict(_target_=cls, **kw)), instantiate=_raises("instantiate"))
    module("util.utils", load_checkpoint=_raises("load_checkpoint"))
    return _load("_reference_swin", os.path.join(ref, "models", "backbones", "swin.py"))


def distance(a32, a64):
    d = a32.double() - a64
    return np.array([d.abs().max().item(), (d.norm() / a64.norm()).item()], dtype=np.float64)


def randomise(module, g, half_grid):
    """Weights at a scale at which every term matters: unit-variance projections, visible biases and tables."""
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if not t.is_floating_point():
                continue
            if name.endswith("relative_position_bias_table"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.5)
            elif t.dim() >= 2:
                t.copy_(torch.randn(t.shape, generator=g) * t[0].numel() ** -0.5)
            elif name.endswith("bias"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.2)
            else:
                t.copy_(1.0 + 0.1 * torch.randn(t.shape, generator=g))
            if half_grid and t.dim() >= 2:
                t.copy_(t.half().float())


def attention_case(swin, name, seed):
    (wh, ww), (sh, sw), (H, W), B = CASES[name]
    g = torch.Generator().manual_seed(seed)
    m = swin.ShiftedWindowAttention(C, [wh, ww], [sh, sw], HEADS).eval()
    randomise(m, g, False)
    x = torch.randn(B, H, W, C, generator=g)
    recorded = []
    original = torch.Tensor.masked_fill

    def recording(self, *args, **kwargs):
        r = original(self, *args, **kwargs)
        recorded.append(r)
        return r
    torch.Tensor.masked_fill = recording                       # the reference's attn_mask is the result of its last masked_fill
    try:
        with torch.no_grad():
            y = m(x)
    finally:
        torch.Tensor.masked_fill = original
    mask = recorded[-1].numpy() if recorded else np.zeros((0,), dtype=np.float32)
    with torch.no_grad():
        y64 = m.double()(x.double())
    m.float()
    return {"cfg": np.array([H, W, wh, ww, sh, sw, B, C, HEADS], dtype=np.int64), "x": x.numpy(), "y": y.numpy(),
            "qkv_w": m.qkv.weight.detach().numpy(), "qkv_b": m.qkv.bias.detach().numpy(), "proj_w": m.proj.weight.detach().numpy(),
            "proj_b": m.proj.bias.detach().numpy(), "table": m.relative_position_bias_table.detach().numpy(),
            "index": m.relative_position_index.numpy(), "mask": mask, "err": distance(y, y64)}


def net_case(swin):
    g = torch.Generator().manual_seed(1616)
    net = swin.SwinTransformer(patch_size=[4, 4], embed_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=[7, 7], mlp_ratio=2.0).eval()
    randomise(net.features, g, True)
    x = torch.randn(2, 3, 36, 68, generator=g)

    def run(model, inp):
        with torch.no_grad():
            f1 = model.features[1](model.features[0](inp))
            f3 = model.features[3](model.features[2](f1))
        return f1, f3
    f1, f3 = run(net, x)
    d1, d3 = run(net.double(), x.double())
    net.float()
    data = {"cfg": np.array([64, 2, 2, 2, 4, 7, 7], dtype=np.int64), "mlp_ratio": np.array(2.0), "x": x.numpy(), "f1": f1.numpy(),
            "f3": f3.numpy(), "err.f1": distance(f1, d1), "err.f3": distance(f3, d3)}
    data.update({f"sd.{k}": (v.half() if v.is_floating_point() and v.dim() >= 2 else v).numpy() for k, v in net.features.state_dict(prefix="features.").items()})
    return data


def key_table(swin, arch):
    cfg = swin.SwinTransformerBackbone.model_arch[arch]
    kwargs = {k: v for k, v in cfg.items() if k not in ("_target_", "url")}
    with torch.device("meta"):
        net = cfg["_target_"](**kwargs)
    sd = {k: v for k, v in net.state_dict().items() if not k.startswith(("norm.", "head."))}
    shapes = np.zeros((len(sd), 4), dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    return {"names": np.array("\n".join(sd)), "shapes": shapes,
            "num_channels": np.array([kwargs["embed_dim"] * 2 ** i for i in (1, 2, 3)], dtype=np.int64)}


def main():
    swin = import_reference()
    out = {}
    for seed, name in enumerate(CASES):
        data = attention_case(swin, name, 1600 + seed)
        out.update({f"att.{name}.{k}": v for k, v in data.items()})
        print(f"{name}: y {data['y'].shape} max |y| {float(np.abs(data['y']).max()):.3f} mask {data['mask'].shape} "
              f"fp32 vs float64: max-abs {data['err'][0]:.3e} rel-L2 {data['err'][1]:.3e}")
    for arch in ("swin_t", "swin_l"):
        data = key_table(swin, arch)
        out.update({f"keys.{arch}.{k}": v for k, v in data.items()})
        print(arch, len(data["shapes"]), "keys", data["num_channels"].tolist())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    data = net_case(swin)
    np.savez_compressed(OUT_NET, **{f"net.{k}": v for k, v in data.items()})
    print(f"wrote {OUT_NET}: {os.path.getsize(OUT_NET)} bytes")
    for k in ("f1", "f3"):
        print(f"net {k}: {data[k].shape} max |.| {float(np.abs(data[k]).max()):.3f} fp32 vs float64: max-abs {data['err.' + k][0]:.3e} "
              f"rel-L2 {data['err.' + k][1]:.3e}")


if __name__ == "__main__":
    main()
