"""CPU-only checks of the host side of the training route that generates the relation bias inside the attention kernels
(csrc/attn_rel.hip + csrc/attn_rel_bwd.hip, relation_detr_amd/attn_rel_train.py): the opt-in switch and how it reaches the
modules, the three C symbols, the workspace size, and the argument refusals, which all happen before any HIP call."""
import ctypes
import os
import re

import pytest
import torch

import relation_detr_amd
from relation_detr_amd import PositionRelationEmbedding, _lib, attn_rel_train, options
from relation_detr_amd.self_attn import RelationSelfAttention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rdetr_relation_attention_boxes_train_bf16", "rdetr_relation_attention_boxes_backward_workspace_bytes",
           "rdetr_relation_attention_boxes_backward_bf16")


def test_rel_train_fused_switch():
    assert options.Options().rel_train_fused is False
    assert options.Options.from_env({}).rel_train_fused is False
    assert options.Options.from_env({"RDETR_REL_TRAIN_FUSED": "1"}).rel_train_fused is True
    assert options.Options.from_env({"RDETR_REL_TRAIN_FUSED": "0"}).rel_train_fused is False
    with pytest.raises(ValueError):
        options.Options.from_env({"RDETR_REL_TRAIN_FUSED": "yes"})


def test_switch_reaches_the_modules():
    from relation_detr_amd.transformer import RelationTransformerDecoder, build_relation_transformer
    mod = RelationSelfAttention(256, 8)
    assert mod.options.rel_train_fused is False
    options.apply(mod, rel_train_fused=True)
    assert mod.options.rel_train_fused is True and mod.options.attn_train_fused is False
    with options.override(rel_train_fused=True):
        assert RelationSelfAttention(256, 8).options.rel_train_fused is True
        net = build_relation_transformer(num_classes=5, d_ffn=32, enc_layers=1, dec_layers=2, num_queries=8)
    assert RelationSelfAttention(256, 8).options.rel_train_fused is False
    assert isinstance(net.decoder, RelationTransformerDecoder) and net.decoder.options.rel_train_fused is True
    attn = [m for m in net.decoder.modules() if isinstance(m, RelationSelfAttention)]
    assert attn and all(m.options.rel_train_fused for m in attn)
    options.apply(net, rel_train_fused=False)
    assert net.decoder.options.rel_train_fused is False and not any(m.options.rel_train_fused for m in attn)


def test_symbols_in_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.rdetr_abi_version() == 3
    for name in ("RelationAttentionBoxesFunction", "relation_attention_boxes_train", "relation_attention_boxes_backward"):
        assert getattr(relation_detr_amd, name) is getattr(attn_rel_train, name) and name in relation_detr_amd.__all__


def test_workspace_bytes():
    ws = _lib.load().rdetr_relation_attention_boxes_backward_workspace_bytes
    for empty in ((0, 8, 10, 10), (2, 0, 10, 10), (2, 8, 0, 10), (2, 8, 10, 0), (-1, 8, 10, 10)):
        assert ws(*empty) == 0, empty
    assert ws(2, 8, 1100, 1100) >= 2 * 8 * 1100 * 4                    # at least Di
    assert ws(2, 8, 1100, 1100) < 4 * 8 * 1100 * 1100                  # and nothing of the size of one image's bias
    sizes_b = [ws(b, 8, 900, 900) for b in (1, 2, 3, 4)]
    sizes_n = [ws(2, 8, n, 900) for n in (1, 16, 17, 300, 900, 1500)]
    assert sizes_b == sorted(sizes_b) and len(set(sizes_b)) == 4
    assert sizes_n == sorted(sizes_n) and sizes_n[0] > 0


ONE = ctypes.c_void_p(256)                       # an aligned non-null dummy: never dereferenced on these paths
ODD = ctypes.c_void_p(258)                       # ... and one that misses every alignment above 2 bytes


def _train(lib, B=1, H=8, D=32, N=10, M=10, F=16, ld=(256,) * 4, ptrs=None):
    q, k, v, src, tgt, w, out, lse = ptrs if ptrs is not None else [ONE] * 8
    return lib.rdetr_relation_attention_boxes_train_bf16(q, k, v, ld[0], ld[1], ld[2], src, tgt, w, None, None, B, H, D, N, M, F, 100.0,
                                                         10000.0, 1e-5, 0.17, out, ld[3], lse, None)


def test_train_forward_argument_refusals():
    lib = _lib.load()
    assert _train(lib, ptrs=[None] * 8) == -1
    for i in range(8):
        ptrs = [ONE] * 8
        ptrs[i] = None
        assert _train(lib, ptrs=ptrs) == -1, i                             # each required pointer, lse included
    assert _train(lib, H=4, D=64) == -2 and _train(lib, D=64, ld=(512,) * 4) == -2 and _train(lib, F=32) == -2
    for shape in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (-1, 10, 10), (1, 10, -3)):
        assert _train(lib, B=shape[0], N=shape[1], M=shape[2]) == -1, shape
    assert _train(lib, H=0) == -1 and _train(lib, F=0) == -1
    for i in range(4):
        ld = [256] * 4
        ld[i] = 248
        assert _train(lib, ld=tuple(ld)) == -1, i                          # shorter than the H * D head span
    for i in (0, 1, 2, 3, 4, 6, 7):                                        # q, k, v, boxes, out, lse misaligned
        ptrs = [ONE] * 8
        ptrs[i] = ODD
        assert _train(lib, ptrs=ptrs) == -2, i
    assert _train(lib, ld=(260, 256, 256, 256)) == -2                      # row stride not a multiple of 8 elements


def _backward(lib, B=1, H=8, D=32, N=10, M=10, F=16, ld=(256,) * 8, ws_bytes=None, ptrs=None, gb=ONE):
    q, k, v, out, lse, dout, src, tgt, w, ws, dq, dk, dv, gw = ptrs if ptrs is not None else [ONE] * 14
    if ws_bytes is None:
        ws_bytes = max(int(lib.rdetr_relation_attention_boxes_backward_workspace_bytes(B, H, N, M)), 0)
    return lib.rdetr_relation_attention_boxes_backward_bf16(
        q, k, v, ld[0], ld[1], ld[2], out, ld[3], lse, dout, ld[4], src, tgt, w, None, None, B, H, D, N, M, F, 100.0, 10000.0, 1e-5,
        0.17, ws, ws_bytes, dq, ld[5], dk, ld[6], dv, ld[7], gw, gb, None)


def test_backward_argument_refusals():
    lib = _lib.load()
    assert _backward(lib, ptrs=[None] * 14) == -1
    for i in range(14):
        ptrs = [ONE] * 14
        ptrs[i] = None
        assert _backward(lib, ptrs=ptrs) == -1, i                          # each required pointer
    big = 1 << 24
    assert _backward(lib, H=4, D=64, ws_bytes=big) == -2
    assert _backward(lib, D=64, ld=(512,) * 8, ws_bytes=big) == -2
    assert _backward(lib, F=32, ws_bytes=big) == -2
    for shape in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (1, -5, 10)):
        assert _backward(lib, B=shape[0], N=shape[1], M=shape[2], ws_bytes=big) == -1, shape
    assert _backward(lib, H=0, ws_bytes=big) == -1 and _backward(lib, F=0, ws_bytes=big) == -1 and _backward(lib, D=0, ws_bytes=big) == -1
    for i in range(8):
        ld = [256] * 8
        ld[i] = 224
        assert _backward(lib, ld=tuple(ld)) == -1, i                       # row stride shorter than the head span
    assert _backward(lib, ws_bytes=16) == -1                               # workspace too small
    for i in range(14):
        ptrs = [ONE] * 14
        ptrs[i] = ODD
        assert _backward(lib, ptrs=ptrs) == -2, i                          # every pointer has an alignment
    assert _backward(lib, gb=ODD) == -2
    assert _backward(lib, ld=(260,) + (256,) * 7) == -2 and _backward(lib, ld=(256,) * 5 + (258, 256, 256)) == -2


def test_ops_refuse_cpu_tensors_and_wrong_arguments(monkeypatch):
    q = torch.zeros(1, 10, 256, dtype=torch.bfloat16)
    boxes, w, b = torch.rand(1, 10, 4), torch.zeros(8, 64, 1, 1), torch.zeros(8)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):
        attn_rel_train.relation_attention_boxes_train(q, q, q, 8, boxes, boxes, w, b)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):
        attn_rel_train.relation_attention_boxes_backward(q, q, q, q, torch.zeros(8, 10), q, 8, boxes, boxes, w, b)
    # dtypes and shapes are checked before the device is touched: make the CPU tensors look like device tensors
    monkeypatch.setattr(attn_rel_train, "_require_device", lambda *t: None)
    with pytest.raises(_lib.RdetrError, match="bfloat16"):
        attn_rel_train.relation_attention_boxes_train(q.float(), q.float(), q.float(), 8, boxes, boxes, w, b)
    with pytest.raises(_lib.RdetrError, match="boxes"):
        attn_rel_train.relation_attention_boxes_train(q, q, q, 8, boxes[:, :9], boxes, w, b)
    with pytest.raises(_lib.RdetrError, match="proj_weight"):
        attn_rel_train.relation_attention_boxes_train(q, q, q, 8, boxes, boxes, w[:, :32], b)
    with pytest.raises(_lib.RdetrError, match="mask"):
        attn_rel_train.relation_attention_boxes_train(q, q, q, 8, boxes, boxes, w, b, mask=torch.zeros(10, 9, dtype=torch.bool))
    with pytest.raises(_lib.RdetrError, match="lse"):
        attn_rel_train.relation_attention_boxes_backward(q, q, q, q, torch.zeros(8, 9), q, 8, boxes, boxes, w, b)


def test_cpu_module_takes_the_old_route_with_the_switch_on(monkeypatch):
    calls = []
    monkeypatch.setattr(attn_rel_train.RelationAttentionBoxesFunction, "apply", lambda *a: calls.append(1))
    materialised = []
    torch.manual_seed(0)
    with options.override(rel_train_fused=True, attn_train_fused=True):
        mod = RelationSelfAttention(256, 8).train()
        rel = PositionRelationEmbedding(16, 8)
    x = torch.randn(1, 6, 256, requires_grad=True)
    recipe = rel.deferred(torch.rand(1, 6, 4), torch.rand(1, 6, 4), None)
    monkeypatch.setattr(recipe, "materialize", lambda: materialised.append(1) or torch.zeros(8, 6, 6))
    with pytest.raises(_lib.RdetrError, match="ROCm device"):          # the old route's bias-softmax kernel: no CPU path
        mod(x, x, x, attn_mask=recipe)
    assert not calls and materialised == [1]
