"""Outputs of the six entry points of the decoder self-attention family (csrc/attn.hip, attn_bwd.hip, attn_rel.hip,
attn_rel_bwd.hip) on seeded inputs, through the public operators, as .npy files under a directory, so that two library builds
can be compared bit for bit after the GPU run:
    RDETR_LIB_PATH=a.so python tools/dump_attn_kernels.py OUT_A ; RDETR_LIB_PATH=b.so python tools/dump_attn_kernels.py OUT_B
    python tools/dump_attn_kernels.py --compare OUT_A OUT_B
Per case: forward without / with the row log-sum-exp of both forwards (out, lse) and both backwards (dq, dk, dv, dbias resp.
grad_weight, grad_bias).  Inputs are generated on the CPU, so they do not depend on the library."""
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, C, F = 8, 256, 16
# name, B, N (queries), M (keys), mask (None | "dn" = denoising blocks | "row" = random + one fully masked row), packed q / k,
# attn.hip with a bias tensor, projection bias
CASES = (
    ("dn_2x1100", 2, 1100, 1100, "dn", True, True, True),
    ("plain_4x900", 4, 900, 900, None, True, True, True),
    ("plain_2x300", 2, 300, 300, None, False, True, True),
    ("edge_37x901", 2, 37, 901, "row", False, True, True),
    ("edge_130x70_nobias", 1, 130, 70, "row", False, False, False),
    ("packed_3x200_nomask_nobias", 3, 200, 200, None, True, False, False),
)


def compare(a, b):
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a, "*.npy")))
    assert names and names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(b, "*.npy"))), "the two directories hold different files"
    bad = [n for n in names if not np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n)), equal_nan=True)]
    print(f"{len(names)} arrays, {len(names) - len(bad)} bit-identical" + (f", DIFFERENT: {bad}" if bad else ""))
    return not bad


def dump(out_dir):
    from relation_detr_amd import _lib, attn_rel_train, ops
    dev = "cuda:0"
    os.makedirs(out_dir, exist_ok=True)
    print("library:", _lib.LIB_PATH)

    def save(name, t):
        if t is None:
            return
        t = t.detach().cpu()
        np.save(os.path.join(out_dir, name + ".npy"), (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy())

    with torch.no_grad():
        for ci, (name, B, N, M, mask_kind, packed, with_bias, with_pb) in enumerate(CASES):
            g = torch.Generator().manual_seed(100 + ci)
            rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)
            if packed:                                  # q / k are the column halves of one projection, as in the decoder
                qk = rnd(B, N, 2 * C)
                q, k = qk[..., :C], qk[..., C:]
            else:
                q, k = rnd(B, N, C), rnd(B, M, C)
            v, dout = rnd(B, M, C), rnd(B, N, C)
            box = lambda n: torch.cat([torch.rand(B, n, 2, generator=g), torch.rand(B, n, 2, generator=g) * 0.4 + 0.02], -1).to(dev)
            src, tgt = box(N), (box(M) if N != M else None)
            tgt = src if tgt is None else tgt
            w = (torch.randn(H, 4 * F, generator=g) * 0.3).to(dev)
            pb = (torch.randn(H, generator=g) * 0.3).to(dev) if with_pb else None
            bias = (torch.randn(B * H, N, M, generator=g) * 2).to(dev) if with_bias else None
            mask = None
            if mask_kind == "dn":                       # denoising-style visibility: the first 200 queries and the rest apart
                i, j = torch.arange(N, device=dev), torch.arange(M, device=dev)
                mask = (i[:, None] < 200) != (j[None, :] < 200)
            elif mask_kind == "row":
                mask = (torch.rand(N, M, generator=g) < 0.3).to(dev)
                mask[min(5, N - 1)] = True              # one fully masked row: NaN out, lse = -inf, zero gradients

            # csrc/attn.hip + csrc/attn_bwd.hip
            save(f"{name}_attn_out", ops.relation_attention(q, k, v, H, bias, mask))
            out, lse = ops.relation_attention_train(q, k, v, H, bias, mask)
            save(f"{name}_attn_train_out", out)
            save(f"{name}_attn_train_lse", lse)
            for tag, need_dbias in (("", False), ("_dbias", True)):
                if need_dbias and bias is None:
                    continue
                dq, dk, dv, dbias = ops.relation_attention_backward(q, k, v, out, lse, dout, H, bias, mask, need_dbias=need_dbias,
                                                                    packed_qk=packed)
                for n_, t in (("dq", dq), ("dk", dk), ("dv", dv), ("dbias", dbias)):
                    save(f"{name}_attn_bwd{tag}_{n_}", t)

            # csrc/attn_rel.hip + csrc/attn_rel_bwd.hip
            save(f"{name}_rel_out", ops.relation_attention_boxes(q, k, v, H, src, tgt, w, pb, mask))
            out, lse = attn_rel_train.relation_attention_boxes_train(q, k, v, H, src, tgt, w, pb, mask)
            save(f"{name}_rel_train_out", out)
            save(f"{name}_rel_train_lse", lse)
            dq, dk, dv, gw, gb = attn_rel_train.relation_attention_boxes_backward(q, k, v, out, lse, dout, H, src, tgt, w, pb, mask,
                                                                                  packed_qk=packed)
            for n_, t in (("dq", dq), ("dk", dk), ("dv", dv), ("grad_weight", gw), ("grad_bias", gb)):
                save(f"{name}_rel_bwd_{n_}", t)
            torch.cuda.synchronize()
    print("wrote", len(glob.glob(os.path.join(out_dir, "*.npy"))), "arrays to", out_dir)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
