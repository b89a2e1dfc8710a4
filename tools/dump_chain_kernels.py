"""Outputs of the decoder chain's two fused kernels (rdetr_query_pos_k256_bf16, rdetr_box_head_k256_bf16) on seeded inputs, as
.npy files under a directory, so that two library builds can be compared bit for bit after the GPU run:
    RDETR_LIB_PATH=a.so python tools/dump_chain_kernels.py OUT_A ; RDETR_LIB_PATH=b.so python tools/dump_chain_kernels.py OUT_B
    python tools/dump_chain_kernels.py --compare OUT_A OUT_B
Inputs are generated on the CPU, so they do not depend on the library."""
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = (1, 37, 600, 1800, 1801, 3600)


def compare(a, b):
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a, "*.npy")))
    assert names and names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(b, "*.npy"))), "the two directories hold different files"
    bad = [n for n in names if not np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n)), equal_nan=True)]
    print(f"{len(names)} arrays, {len(names) - len(bad)} bit-identical" + (f", DIFFERENT: {bad}" if bad else ""))
    return not bad


def dump(out_dir):
    from relation_detr_amd import _lib, ops
    from relation_detr_amd.transformer import MLP
    dev = "cuda:0"
    os.makedirs(out_dir, exist_ok=True)
    print("library:", _lib.LIB_PATH)
    torch.manual_seed(0)
    head, scale, box = MLP(512, 256, 256, 2), MLP(256, 256, 256, 2), MLP(256, 256, 4, 3)
    with torch.no_grad():
        box.layers[2].weight.copy_(torch.randn(4, 256) * 0.05)             # the reference initialises the last layer with zeros
        for l in (*head.layers, *scale.layers, *box.layers):
            l.bias.copy_(torch.randn(l.bias.shape) * 0.1)
    head, scale, box = (m.to(dev).to(torch.bfloat16) for m in (head, scale, box))
    g = torch.Generator().manual_seed(1)

    def save(name, t):
        t = t.detach().cpu()
        np.save(os.path.join(out_dir, name + ".npy"), (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy())

    with torch.no_grad():
        for rows in ROWS:
            emb = torch.randn(rows, 512, generator=g).to(torch.bfloat16).to(dev)
            q = torch.randn(rows, 256, generator=g).to(torch.bfloat16).to(dev)
            xa = torch.randn(rows, 256, generator=g).to(torch.bfloat16).to(dev)
            xb = torch.randn(rows, 256, generator=g).to(torch.bfloat16).to(dev)
            ref = torch.rand(rows, 4, generator=g).to(dev)
            logit = (torch.randn(rows, 4, generator=g) * 2).to(dev)
            for tag, sc in (("layer0", None), ("scaled", scale.layers)):
                pos, qpp = ops.query_pos_k256(emb, q, head.layers, sc)
                save(f"qpos_{tag}_{rows}_pos", pos)
                save(f"qpos_{tag}_{rows}_qpp", qpp)
            a, b = ops.box_head_k256(xa, xb, box.layers, ref)
            save(f"box_{rows}_a", a)
            save(f"box_{rows}_b", b)
            save(f"box_{rows}_logit", ops.box_head_k256(xa, None, box.layers, logit, reference_is_logit=True))
        torch.cuda.synchronize()
    print("wrote", len(glob.glob(os.path.join(out_dir, "*.npy"))), "arrays to", out_dir)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
