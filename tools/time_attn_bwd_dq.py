#!/usr/bin/env python3
"""Backward of the fused self-attention with dbias, its dQ kernel recomputing dS (mode 1, the shipped choice) against reading dS
back from dbias (mode 2), alternating; median of the hipEvent-timed reps.  Needs the development library:

    make -C relation_detr_amd/csrc dev && RDETR_LIB_PATH=relation_detr_amd/librelation_detr_amd_dev.so python3 tools/time_attn_bwd_dq.py
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import _lib, ops  # noqa: E402

lib = _lib.load()
dev = "cuda:0"
for B, N in ((2, 1100), (4, 900), (2, 300)):
    g = torch.Generator().manual_seed(0)
    qk = torch.randn(B, N, 512, generator=g).to(torch.bfloat16).to(dev)
    v = torch.randn(B, N, 256, generator=g).to(torch.bfloat16).to(dev)
    bias = (torch.rand(16 if B == 2 else 32, N, N, generator=g) * 3).to(dev)
    do = torch.randn(B, N, 256, generator=g).to(torch.bfloat16).to(dev)
    q, k = qk[..., :256], qk[..., 256:]
    out, lse = ops.relation_attention_train(q, k, v, 8, bias)
    res = {}
    ref = None
    for mode in (1, 2, 1, 2, 1, 2):
        lib.rdetr_dev_set_attn_bwd_dq(mode)
        ts = []
        for i in range(13):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = ops.relation_attention_backward(q, k, v, out, lse, do, 8, bias, need_dbias=True, packed_qk=True)
            e1.record(); torch.cuda.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1))
        res.setdefault(mode, []).extend(ts)
        if ref is None:
            ref = r[0].float()
        diff = (r[0].float() - ref).abs().max().item()
    print(f"B={B} N={N} backward with dbias: dq recompute {statistics.median(res[1]):.3f} ms, dq read-back {statistics.median(res[2]):.3f} ms, max|dq diff| {diff:.2e}")
