"""Host-side contract of the decoder-chain absorptions (no GPU): the two new entry points refuse bad arguments before any HIP call,
and ``ops.query_pos_k256(in_proj=...)`` / ``ops.box_head_k256(class_head=...)`` refuse wrong shapes and dtypes with RdetrError."""
import ctypes

import pytest
import torch

from relation_detr_amd import _lib, ops
from relation_detr_amd.transformer import MLP

BF = torch.bfloat16


def test_c_abi_argument_validation_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                       # an aligned non-null dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(24)
    qp = lib.rdetr_query_pos_inproj_k256_bf16

    def qpos(emb=one, lde=512, ldq=256, wq=one, bias=one, M=4, qk=one, ldqk=512, v=one, ldv=256, scale=(None,) * 4):
        return qp(emb, lde, one, ldq, one, one, one, one, one, *scale, wq, one, one, bias, M, one, one, qk, ldqk, v, ldv, None)
    assert qpos(M=0) == 0 and qpos(M=-1) == -1
    assert qpos(ldqk=511) == -1 and qpos(ldv=255) == -1 and qpos(lde=511) == -1                 # a row stride below a row
    assert qpos(ldqk=516) == -2 and qpos(ldv=260) == -2                                          # rows not 16-byte multiples
    assert qpos(wq=None) == -1 and qpos(bias=None) == -1 and qpos(qk=None) == -1 and qpos(v=None) == -1
    assert qpos(qk=odd) == -2 and qpos(v=odd) == -2 and qpos(wq=odd) == -2                       # misaligned
    assert qpos(scale=(one, None, one, one)) == -1                                               # half a scale branch
    bh = lib.rdetr_box_head_cls_k256_bf16

    def box(xa=one, lda=256, pwc=one, bc=one, C=91, M=4, cls=one, ldc=91):
        return bh(xa, lda, None, 0, one, one, one, one, one, one, one, 0, 1e-3, pwc, bc, C, M, one, None, cls, ldc, None)
    assert box(M=0) == 0 and box(M=-1) == -1
    assert box(C=0) == -1 and box(C=257, ldc=257) == -2 and box(ldc=90) == -1
    assert box(pwc=None) == -1 and box(bc=None) == -1 and box(cls=None) == -1
    assert box(pwc=odd) == -2 and box(cls=ctypes.c_void_p(17)) == -2 and box(lda=260) == -2


def test_in_proj_keyword_is_checked_before_anything_runs():
    head = MLP(512, 256, 256, 2).to(BF)
    emb, query = torch.zeros(4, 512, dtype=BF), torch.zeros(4, 256, dtype=BF)
    w, b = torch.zeros(768, 256, dtype=BF), torch.zeros(768, dtype=BF)
    for bad in ({"weight": w[:512], "bias": b}, {"weight": w.float(), "bias": b}, {"weight": w, "bias": b.float()},
                {"weight": w, "bias": b[:256]}, {"weight": w}, {"bias": b},
                {"weight": w, "bias": b, "qk": torch.zeros(4, 256, dtype=BF)}, {"weight": w, "bias": b, "qk": torch.zeros(3, 512, dtype=BF)},
                {"weight": w, "bias": b, "v": torch.zeros(4, 256)}, {"weight": w, "bias": b, "v": torch.zeros(4, 260, dtype=BF)[:, 4:]}):
        with pytest.raises(_lib.RdetrError, match="in_proj"):
            ops.query_pos_k256(emb, query, head.layers, None, in_proj=bad)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):      # a well-formed one gets as far as the device check
        ops.query_pos_k256(emb, query, head.layers, None, in_proj={"weight": w, "bias": b})


def test_class_head_keyword_is_checked_before_anything_runs():
    head = MLP(256, 256, 4, 3).to(BF)
    xa, ref = torch.zeros(4, 256, dtype=BF), torch.full((4, 4), 0.5)
    lin = torch.nn.Linear(256, 91).to(BF)
    for bad in ({"linear": torch.nn.Linear(256, 91)}, {"linear": torch.nn.Linear(128, 91).to(BF)}, {"linear": torch.nn.Linear(256, 257).to(BF)},
                {"linear": torch.nn.Linear(256, 91, bias=False).to(BF)}, {}, {"linear": lin, "out": torch.zeros(4, 92, dtype=BF)},
                {"linear": lin, "out": torch.zeros(3, 91, dtype=BF)}, {"linear": lin, "out": torch.zeros(4, 91)}):
        with pytest.raises(_lib.RdetrError, match="class_head"):
            ops.box_head_k256(xa, None, head.layers, ref, class_head=bad)
    with pytest.raises(_lib.RdetrError, match="ROCm device"):
        ops.box_head_k256(xa, None, head.layers, ref, class_head={"linear": lin})
