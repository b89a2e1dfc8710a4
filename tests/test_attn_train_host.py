"""CPU-only checks of the fused bf16 self-attention training route's host side: the opt-in switch, the module's options object,
and the argument refusals of the C entry points and the ops, which all happen before any HIP call."""
import ctypes

import pytest
import torch

from relation_detr_amd import _lib, ops, options
from relation_detr_amd.self_attn import RelationSelfAttention


def test_attn_train_fused_switch():
    assert options.Options().attn_train_fused is False
    assert options.Options.from_env({}).attn_train_fused is False
    assert options.Options.from_env({"RDETR_ATTN_TRAIN_FUSED": "1"}).attn_train_fused is True
    assert options.Options.from_env({"RDETR_ATTN_TRAIN_FUSED": "0"}).attn_train_fused is False
    with pytest.raises(ValueError):
        options.Options.from_env({"RDETR_ATTN_TRAIN_FUSED": "on"})


def test_self_attention_module_holds_options():
    mod = RelationSelfAttention(256, 8)
    assert isinstance(mod.options, options.Options)
    assert mod.options.attn_train_fused is False
    options.apply(mod, attn_train_fused=True)
    assert mod.options.attn_train_fused is True
    with options.override(attn_train_fused=True):
        assert RelationSelfAttention(256, 8).options.attn_train_fused is True
    assert RelationSelfAttention(256, 8).options.attn_train_fused is False


ONE = ctypes.c_void_p(256)                       # an aligned non-null dummy: never dereferenced on these paths


def _train(lib, B=1, H=8, D=32, N=10, M=10, ld=(256, 256, 256, 256), ptrs=None):
    q, k, v, out, lse = ptrs if ptrs is not None else [ONE] * 5
    return lib.rdetr_relation_attention_train_bf16(q, k, v, ld[0], ld[1], ld[2], None, None, B, H, D, N, M, 0.17, out, ld[3], lse,
                                                    None)


def test_train_forward_argument_refusals():
    lib = _lib.load()
    assert _train(lib, ptrs=[None] * 5) == -1                              # null pointers
    assert _train(lib, ptrs=[ONE, ONE, ONE, ONE, None]) == -1              # null lse
    assert _train(lib, D=64, ld=(512,) * 4) == -2                          # head dim
    for shape in ((0, 8, 10, 10), (1, 0, 10, 10), (1, 8, 0, 10), (1, 8, 10, 0), (-1, 8, 10, 10), (1, 8, 10, -3)):
        B, H, N, M = shape
        assert _train(lib, B=B, H=H, N=N, M=M) == -1, shape                # non-positive sizes
    for i in range(4):
        ld = [256] * 4
        ld[i] = 248                                                        # shorter than the H * D = 256 head span
        assert _train(lib, ld=tuple(ld)) == -1, i


def _backward(lib, B=1, H=8, D=32, N=10, M=10, ld=(256,) * 8, ws_bytes=None, ptrs=None, dbias=None):
    q, k, v, out, lse, dout, ws, dq, dk, dv = ptrs if ptrs is not None else [ONE] * 10
    if ws_bytes is None:
        ws_bytes = max(int(lib.rdetr_relation_attention_backward_workspace_bytes(B, H, N)), 0)
    return lib.rdetr_relation_attention_backward_bf16(q, k, v, ld[0], ld[1], ld[2], out, ld[3], lse, dout, ld[4], None, None,
                                                      B, H, D, N, M, 0.17, ws, ws_bytes, dq, ld[5], dk, ld[6], dv, ld[7], dbias, None)


def test_backward_argument_refusals():
    lib = _lib.load()
    assert lib.rdetr_relation_attention_backward_workspace_bytes(2, 8, 1100) >= 2 * 8 * 1100 * 4
    assert lib.rdetr_relation_attention_backward_workspace_bytes(0, 8, 1100) == 0
    assert _backward(lib, ptrs=[None] * 10) == -1                          # null pointers
    for i in range(10):
        ptrs = [ONE] * 10
        ptrs[i] = None
        assert _backward(lib, ptrs=ptrs) == -1, i                          # each required pointer
    assert _backward(lib, D=64, ld=(512,) * 8, ws_bytes=1 << 20) == -2     # head dim
    for shape in ((0, 8, 10, 10), (1, 0, 10, 10), (1, 8, 0, 10), (1, 8, 10, 0), (1, 8, -5, 10)):
        B, H, N, M = shape
        assert _backward(lib, B=B, H=H, N=N, M=M, ws_bytes=1 << 20) == -1, shape
    for i in range(8):
        ld = [256] * 8
        ld[i] = 224
        assert _backward(lib, ld=tuple(ld)) == -1, i                       # row stride shorter than the head span
    assert _backward(lib, ws_bytes=16) == -1                               # workspace too small


def test_ops_refuse_cpu_and_wrong_arguments():
    q = torch.zeros(1, 10, 256, dtype=torch.bfloat16)
    with pytest.raises(_lib.RdetrError):
        ops.relation_attention_train(q, q, q, 8)                           # CPU tensors
    with pytest.raises(_lib.RdetrError):
        ops.relation_attention_backward(q, q, q, q, torch.zeros(8, 10), q, 8)
    assert hasattr(ops, "RelationAttentionFunction")
    if not torch.cuda.is_available():
        return
    dev = "cuda"
    qd = q.to(dev)
    with pytest.raises(_lib.RdetrError):
        ops.relation_attention_train(qd.float(), qd.float(), qd.float(), 8)                             # not bf16
    with pytest.raises(_lib.RdetrError):
        ops.relation_attention_train(qd, qd, qd, 8, bias=torch.zeros(8, 10, 9, device=dev))          # bias shape
    with pytest.raises(_lib.RdetrError):
        ops.relation_attention_train(qd, qd, qd, 8, mask=torch.zeros(10, 9, dtype=torch.bool, device=dev))   # mask shape


def test_ops_refuse_non_bf16_and_wrong_shapes_before_any_launch(monkeypatch):
    # the ops check dtypes and shapes before touching the device: make the CPU tensors look like device tensors
    monkeypatch.setattr(ops, "_require_device", lambda *t: None)
    q = torch.zeros(1, 10, 256, dtype=torch.bfloat16)
    with pytest.raises(_lib.RdetrError, match="bfloat16"):
        ops.relation_attention_train(q.float(), q.float(), q.float(), 8)
    with pytest.raises(_lib.RdetrError, match="bias"):
        ops.relation_attention_train(q, q, q, 8, bias=torch.zeros(8, 10, 9))
    with pytest.raises(_lib.RdetrError, match="bias"):
        ops.relation_attention_train(q, q, q, 8, bias=torch.zeros(8, 10, 10, dtype=torch.bfloat16))
    with pytest.raises(_lib.RdetrError, match="mask"):
        ops.relation_attention_train(q, q, q, 8, mask=torch.zeros(10, 9, dtype=torch.bool))
    with pytest.raises(_lib.RdetrError, match="mask"):
        ops.relation_attention_backward(q, q, q, q, torch.zeros(8, 10), q, 8, mask=torch.zeros(9, 10, dtype=torch.bool))
    with pytest.raises(_lib.RdetrError, match="lse"):
        ops.relation_attention_backward(q, q, q, q, torch.zeros(8, 9), q, 8)
