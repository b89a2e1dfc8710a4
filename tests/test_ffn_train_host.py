"""CPU-only checks of the host side of the fused training route of the feed-forward block (csrc/ffn.hip,
relation_detr_amd/ffn_train.py): the opt-in switch and how it reaches the encoder layers, the two C symbols, every argument refusal
(all of them happen before any HIP call), and that a CPU module with the switch on computes what it computes with the switch off."""
import ctypes
import os
import re

import pytest
import torch

import relation_detr_amd
from relation_detr_amd import _lib, ffn_train, options
from relation_detr_amd.transformer import RelationTransformerEncoderLayer, build_relation_transformer, feed_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rdetr_ffn_k256_train_bf16", "rdetr_ffn_k256_backward_bf16")


def test_ffn_train_fused_switch():
    assert options.Options().ffn_train_fused is False
    assert options.Options.from_env({}).ffn_train_fused is False
    assert options.Options.from_env({"RDETR_FFN_TRAIN_FUSED": "1"}).ffn_train_fused is True
    assert options.Options.from_env({"RDETR_FFN_TRAIN_FUSED": "0"}).ffn_train_fused is False
    with pytest.raises(ValueError):
        options.Options.from_env({"RDETR_FFN_TRAIN_FUSED": "on"})


def test_switch_reaches_the_encoder_layers():
    layer = RelationTransformerEncoderLayer(256, 64)
    assert layer.options.ffn_train_fused is False
    options.apply(layer, ffn_train_fused=True)
    assert layer.options.ffn_train_fused is True and layer.options.ffn_fused is True
    with options.override(ffn_train_fused=True):
        assert RelationTransformerEncoderLayer(256, 64).options.ffn_train_fused is True
        net = build_relation_transformer(num_classes=5, d_ffn=32, enc_layers=2, dec_layers=1, num_queries=8)
    assert RelationTransformerEncoderLayer(256, 64).options.ffn_train_fused is False
    layers = [m for m in net.modules() if isinstance(m, RelationTransformerEncoderLayer)]
    assert len(layers) == 2 and all(m.options.ffn_train_fused for m in layers)
    options.apply(net, ffn_train_fused=False)
    assert not any(m.options.ffn_train_fused for m in layers)


def test_symbols_in_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.rdetr_abi_version() == 3
    for name in ("FeedForwardFunction", "ffn_k256_train", "ffn_k256_backward"):
        assert getattr(relation_detr_amd, name) is getattr(ffn_train, name) and name in relation_detr_amd.__all__


ONE = ctypes.c_void_p(256)                       # an aligned non-null dummy: never dereferenced on these paths
ODD = ctypes.c_void_p(264)                       # ... and one that is 8- but not 16-byte aligned


def _train(lib, M=100, F=128, ld=(256, 256, None), ptrs=None):
    x, packed, b1, b2, out, hid = ptrs if ptrs is not None else [ONE] * 6
    ldx, ldo, ldh = ld
    return lib.rdetr_ffn_k256_train_bf16(x, ldx, packed, b1, b2, M, F, out, ldo, hid, F if ldh is None else ldh, None)


def test_train_forward_argument_refusals():
    lib = _lib.load()
    for i in range(6):
        ptrs = [ONE] * 6
        ptrs[i] = None
        assert _train(lib, ptrs=ptrs) == -1, i                             # each pointer, the hidden activations included
    assert _train(lib, F=96) == -2 and _train(lib, F=4160) == -2           # F % 64, F > 4096
    assert _train(lib, F=0) == -1 and _train(lib, F=-64) == -1
    assert _train(lib, M=-1) == -1
    assert _train(lib, M=0) == 0 and _train(lib, M=0, ptrs=[None] * 6) == 0
    assert _train(lib, ld=(248, 256, None)) == -1 and _train(lib, ld=(256, 248, None)) == -1 and _train(lib, ld=(256, 256, 120)) == -1
    assert _train(lib, ld=(260, 256, None)) == -2 and _train(lib, ld=(256, 260, None)) == -2 and _train(lib, ld=(256, 256, 132)) == -2
    for i in (0, 1, 4, 5):                                                 # x, packed, out, hid misaligned
        ptrs = [ONE] * 6
        ptrs[i] = ODD
        assert _train(lib, ptrs=ptrs) == -2, i
    # hid is addressed with 32-bit byte offsets whose top bit is taken: M * ldh * 2 must stay below 2^31
    assert _train(lib, M=(1 << 31) // (2 * 2048), F=2048) == -2
    assert _train(lib, M=1 << 20, F=64, ld=(256, 256, 1024)) == -2
    assert _train(lib, M=1 << 40, F=64) == -2


def _backward(lib, M=100, F=128, ld=(256, None, None, 256), ptrs=None):
    dy, packed, hid, dh, dx = ptrs if ptrs is not None else [ONE] * 5
    lddy, ldh, ldd, lddx = ld
    return lib.rdetr_ffn_k256_backward_bf16(dy, lddy, packed, hid, F if ldh is None else ldh, M, F, dh, F if ldd is None else ldd, dx,
                                            lddx, None)


def test_backward_argument_refusals():
    lib = _lib.load()
    for i in range(5):
        ptrs = [ONE] * 5
        ptrs[i] = None
        assert _backward(lib, ptrs=ptrs) == -1, i
    assert _backward(lib, F=96) == -2 and _backward(lib, F=4160) == -2
    assert _backward(lib, F=0) == -1
    assert _backward(lib, M=-5) == -1
    assert _backward(lib, M=0) == 0 and _backward(lib, M=0, ptrs=[None] * 5) == 0
    for i, short in enumerate((248, 120, 120, 248)):                       # dy, hid, dh, dx rows shorter than a row
        ld = [256, None, None, 256]
        ld[i] = short
        assert _backward(lib, ld=tuple(ld)) == -1, i
    for i, odd in enumerate((260, 132, 132, 260)):                         # ... or not a multiple of 8 elements
        ld = [256, None, None, 256]
        ld[i] = odd
        assert _backward(lib, ld=tuple(ld)) == -2, i
    for i in range(5):
        ptrs = [ONE] * 5
        ptrs[i] = ODD
        assert _backward(lib, ptrs=ptrs) == -2, i                          # every pointer is read or written 16 bytes at a time
    assert _backward(lib, M=(1 << 31) // (2 * 2048), F=2048) == -2         # hid and dh
    assert _backward(lib, M=1 << 20, F=64, ld=(256, 1024, None, 256)) == -2    # hid alone
    assert _backward(lib, M=1 << 20, F=64, ld=(256, None, 1024, 256)) == -2    # dh alone


def test_ops_refuse_cpu_tensors_and_wrong_arguments(monkeypatch):
    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    w1, b1 = torch.zeros(64, 256, dtype=torch.bfloat16), torch.zeros(64, dtype=torch.bfloat16)
    w2, b2 = torch.zeros(256, 64, dtype=torch.bfloat16), torch.zeros(256, dtype=torch.bfloat16)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):
        ffn_train.ffn_k256_train(x, w1, b1, w2, b2)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):
        ffn_train.ffn_k256_backward(x, torch.zeros(4, 64, dtype=torch.bfloat16), w1, w2)
    assert ffn_train.ffn_train_supported(x, w1, b1, w2, b2) is False       # not on a device
    monkeypatch.setattr(ffn_train, "_require_device", lambda *t: None)
    with pytest.raises(_lib.RdetrError, match="w1"):
        ffn_train.ffn_k256_backward(x, torch.zeros(4, 64, dtype=torch.bfloat16), w1.float(), w2)
    with pytest.raises(_lib.RdetrError, match="hid"):
        ffn_train.ffn_k256_backward(x, torch.zeros(3, 64, dtype=torch.bfloat16), w1, w2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_feed_forward_is_unchanged_by_the_switch(dtype, monkeypatch):
    calls = []
    monkeypatch.setattr(ffn_train.FeedForwardFunction, "apply", lambda *a: calls.append(1))
    torch.manual_seed(0)
    layer = RelationTransformerEncoderLayer(256, 128).to(dtype)
    x0 = torch.randn(2, 40, 256).to(dtype)
    results = []
    for on in (False, True):
        options.apply(layer, ffn_train_fused=on)
        layer.zero_grad()
        x = x0.clone().requires_grad_()
        out = feed_forward(layer.linear1, layer.linear2, x, layer.options)
        out.square().sum().backward()
        results.append([out.detach(), x.grad] + [p.grad.clone() for p in (layer.linear1.weight, layer.linear1.bias, layer.linear2.weight,
                                                                            layer.linear2.bias)])
    assert not calls
    for a, b in zip(*results):
        assert torch.equal(a, b)
