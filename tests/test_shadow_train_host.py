"""CPU test of the shadow checkers of the training entries outside ops.py (tests/shadow.py, TRAIN_ENTRIES).  Needs neither a GPU
nor the built library: each entry's result is formed by the unfused torch sequence from bf16 (LayerNorm: fp32 too) tensors, in
fp32 arithmetic, rounded where the kernel stores.  Every Cmp of the checker must pass on that -- the float64 reference alone
stays inside its own bounds at these shapes -- and each corruption below must fail it.

Shapes: FFN 37 rows x F = 64; LayerNorm 5 and 300 rows; attention B = 2, N = M = 37 with a block mask and one fully masked row;
MSDA levels [(9, 7), (5, 4)], B = 2, one padded image.
"""
import math

import pytest
import torch

import shadow
from oracle import torch_ref

BF = torch.bfloat16


def _rand(g, *shape, dtype=BF, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _failing(key, args, res):
    with torch.no_grad():
        out = [shadow._compare(c) for c in shadow.TRAIN_ENTRIES[key](args, res)]
    assert out and sum(n for _, _, n, _ in out) > 0
    return [(w, f, r) for r, f, _, w in out if f or not math.isfinite(r)]


def _passes(key, args, res):
    bad = _failing(key, args, res)
    assert not bad, (key, bad)


def _fails(key, args, res, label):
    bad = _failing(key, args, res)
    assert bad, f"{key}: the checker accepted `{label}`"
    return bad


def _scale_column(t, col=3):
    t = t.clone()
    t[..., col] = (t[..., col].float() * (1 + 2.0 ** -5)).to(t.dtype)
    return t


def _swap_blocks(t):
    """rows 0-15 and 16-31 of the flattened [rows, C] view exchanged"""
    t2 = t.clone().reshape(-1, t.shape[-1])
    t2[0:16], t2[16:32] = t.reshape(-1, t.shape[-1])[16:32], t.reshape(-1, t.shape[-1])[0:16]
    return t2.reshape(t.shape)


# ------------------------------------------------------------------------------------------------------------------ FFN
@pytest.fixture(scope="module")
def ffn():
    g = torch.Generator().manual_seed(1)
    rows, F = 37, 64
    x, dy = _rand(g, rows, 256), _rand(g, rows, 256)
    w1, b1 = _rand(g, F, 256, scale=256 ** -0.5), _rand(g, F, scale=0.1)
    w2, b2 = _rand(g, 256, F, scale=F ** -0.5), _rand(g, 256, scale=0.1)
    hid = torch.relu(x.float() @ w1.float().t() + b1.float()).to(BF)
    out = (hid.float() @ w2.float().t() + b2.float()).to(BF)
    raw = (dy.float() @ w2.float()).to(BF)
    dh = raw * (hid > 0)
    dx = (dh.float() @ w1.float()).to(BF)
    return dict(fwd=dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2), bwd=dict(dy=dy, hid=hid, w1=w1, w2=w2), out=out, hid=hid, dh=dh, dx=dx, raw=raw)


def test_ffn_checkers(ffn):
    fwd, bwd = "ffn_train.ffn_k256_train", "ffn_train.ffn_k256_backward"
    _passes(fwd, ffn["fwd"], (ffn["out"], ffn["hid"]))
    _passes(bwd, ffn["bwd"], (ffn["dx"], ffn["dh"]))
    assert "out" in _fails(fwd, ffn["fwd"], (_scale_column(ffn["out"]), ffn["hid"]), "out column scaled")[0][0]
    assert "hid" in _fails(fwd, ffn["fwd"], (ffn["out"], _scale_column(ffn["hid"], 5)), "hid column scaled")[0][0]
    assert "hid" in _fails(fwd, ffn["fwd"], (ffn["out"], _swap_blocks(ffn["hid"])), "hid blocks swapped")[0][0]
    assert "dx" in _fails(bwd, ffn["bwd"], (_scale_column(ffn["dx"]), ffn["dh"]), "dx column scaled")[0][0]
    assert "dx" in _fails(bwd, ffn["bwd"], (_swap_blocks(ffn["dx"]), ffn["dh"]), "dx blocks swapped")[0][0]
    assert (ffn["hid"] <= 0).any() and (ffn["raw"][ffn["hid"] <= 0] != 0).any()
    dx_raw = (ffn["raw"].float() @ ffn["fwd"]["w1"].float()).to(BF)       # consistent with the unzeroed dH: only dH can fail
    bad = _fails(bwd, ffn["bwd"], (dx_raw, ffn["raw"]), "dH not zeroed where hid <= 0")
    assert len(bad) == 1 and "dH" in bad[0][0]
    one = ffn["dh"].clone()                                               # a single dead unit given 2^-120: exact zero is asked
    i = (ffn["hid"] <= 0).nonzero()[0]
    one[i[0], i[1]] = 2.0 ** -120
    assert "dH" in _fails(bwd, ffn["bwd"], (ffn["dx"], one), "one dead unit not zero")[0][0]


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_case(dtype, rows, residual):
    g = torch.Generator().manual_seed(rows + (7 if residual else 0))
    x = _rand(g, rows, 256, dtype=dtype) + 0.5
    r = _rand(g, rows, 256, dtype=dtype, scale=2.0) if residual else None
    w, b = (1 + 0.2 * torch.randn(256, generator=g)).to(dtype), (0.2 * torch.randn(256, generator=g)).to(dtype)
    dy = _rand(g, rows, 256, dtype=dtype)
    return x, r, w, b, dy


def _ln_torch(x, r, w, b, dy, eps=1e-5):
    """torch's layer_norm and its autograd in fp32 arithmetic on the fp32 sum (the kernels never store the sum), results rounded
    to x's dtype where the kernels store them; the statistics stay fp32."""
    s = (x.float() if r is None else x.float() + r.float()).requires_grad_(True)
    wf, bfl = w.float().requires_grad_(True), b.float().requires_grad_(True)
    out = torch.nn.functional.layer_norm(s, (256,), wf, bfl, eps)
    out.backward(dy.float())
    sd = s.detach()
    stats = torch.stack([sd.mean(-1), (sd.var(-1, unbiased=False) + eps).rsqrt()], -1)
    return out.detach().to(x.dtype), stats, s.grad.to(x.dtype), wf.grad.to(x.dtype), bfl.grad.to(x.dtype)


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("rows", [5, 300])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_layer_norm_checkers(dtype, rows, residual):
    fwd, bwd = "ln_train.add_layer_norm_train", "ln_train.add_layer_norm_backward"
    x, r, w, b, dy = _ln_case(dtype, rows, residual)
    out, stats, dx, dg, db = _ln_torch(x, r, w, b, dy)
    a_f = dict(x=x, residual=r, weight=w, bias=b, eps=1e-5)
    a_b = dict(dy=dy, x=x, residual=r, stats=stats, weight=w, need_params=True)
    _passes(fwd, a_f, (out, stats))
    _passes(bwd, a_b, (dx, dg, db))
    _passes(bwd, dict(a_b, need_params=False), (dx, None, None))
    assert "out" in _fails(fwd, a_f, (_scale_column(out), stats), "out column scaled")[0][0]
    bumped = stats.clone()
    bumped[rows // 2, 1] *= 1 + 2.0 ** -14
    assert "rstd" in _fails(fwd, a_f, (out, bumped), "one rstd off by 2^-14")[0][0]
    assert "dx" in _fails(bwd, a_b, (_scale_column(dx), dg, db), "dx column scaled")[0][0]
    big = int(dg.float().abs().argmax())
    dg2 = dg.clone()
    dg2[big] = (dg2[big].float() * (1 + 2.0 ** -5)).to(dtype)
    assert "dgamma" in _fails(bwd, a_b, (dx, dg2, db), "dgamma channel scaled")[0][0]
    if rows >= 32:
        assert "dx" in _fails(bwd, a_b, (_swap_blocks(dx), dg, db), "dx blocks swapped")[0][0]
    if residual:
        alone = _ln_torch(x, None, w, b, dy)[2]
        assert "dx" in _fails(bwd, a_b, (alone, dg, db), "dx taken from x alone")[0][0]


# ------------------------------------------------------------------------------------------------------------ attention
@pytest.fixture(scope="module")
def attn():
    g = torch.Generator().manual_seed(3)
    B, N, H, C, D = 2, 37, 8, 256, 32
    q, k, v, dout = (_rand(g, B, N, C) for _ in range(4))
    boxes = lambda: torch.cat([torch.rand(B, N, 2, generator=g), torch.rand(B, N, 2, generator=g) * 0.4 + 0.02], -1)     # noqa: E731
    src, tgt = boxes(), boxes()
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(64, H, 1)
    w, pb = conv.weight.detach().to(BF), conv.bias.detach().to(BF)
    mask = torch.zeros(N, N, dtype=torch.bool)
    mask[:12, 20:] = True                                                   # a block, as the denoising groups make
    mask[20:, :12] = True
    mask[7, :] = True                                                       # one query sees no key
    scale = D ** -0.5
    # the unfused sequence in fp32, the sine features rounded to bf16 as the kernels hold them
    feat = torch_ref.sine_embed(torch_ref.box_rel_encoding(src, tgt)).to(BF).float()                  # [B, N, M, 64]
    pre = torch.einsum("bnmc,hc->bhnm", feat, w.float().reshape(H, -1)) + pb.float().view(1, H, 1, 1)
    heads = lambda t: t.float().view(B, N, H, D).transpose(1, 2)                                     # noqa: E731
    s = heads(q) @ heads(k).transpose(-1, -2) * scale + pre.relu()
    s = s.masked_fill(mask, float("-inf"))
    p = s.softmax(-1)
    out = (p @ heads(v)).transpose(1, 2).reshape(B, N, C).to(BF)
    lse2 = (torch.logsumexp(s, -1) / math.log(2.0)).reshape(B * H, N)
    p = torch.nan_to_num(p, nan=0.0)
    do = heads(dout)
    ds = torch.where(p > 0, p * (do @ heads(v).transpose(-1, -2) - (do * heads(out)).sum(-1, keepdim=True)), torch.zeros_like(p))
    back = lambda t: t.transpose(1, 2).reshape(B, N, C).to(BF)                                       # noqa: E731
    dq, dk, dv = back(ds @ heads(k) * scale), back(ds.transpose(-1, -2) @ heads(q) * scale), back(p.transpose(-1, -2) @ do)
    dsa = ds * (pre > 0)
    gw, gb = torch.einsum("bhnm,bnmc->hc", dsa, feat), dsa.sum(dim=(0, 2, 3))
    common = dict(q=q, k=k, v=v, num_heads=H, src_boxes=src, tgt_boxes=tgt, proj_weight=w, proj_bias=pb, mask=mask, scale=scale,
                  num_pos_feats=16, temperature=10000.0, rel_scale=100.0, eps=1e-5)
    return dict(fwd=common, bwd=dict(common, out=out, lse2=lse2, dout=dout, packed_qk=False), out=out, lse2=lse2,
                grads=(dq, dk, dv, gw, gb, None))


def test_attention_checkers(attn):
    fwd, bwd = "attn_rel_train._relation_attention_boxes_train", "attn_rel_train._relation_attention_boxes_backward"
    out, lse2, grads = attn["out"], attn["lse2"], attn["grads"]
    assert torch.isnan(out[:, 7]).all() and torch.isneginf(lse2.view(2, 8, 37)[:, :, 7]).all()
    _passes(fwd, attn["fwd"], (out, lse2))
    _passes(bwd, attn["bwd"], grads)
    assert "out" in _fails(fwd, attn["fwd"], (_scale_column(out), lse2), "out column scaled")[0][0]
    assert "lse" in _fails(fwd, attn["fwd"], (out, lse2 + 2e-3 / math.log(2.0)), "lse shifted by 2e-3")[0][0]
    for i, name in enumerate(("dq", "dk", "dv")):
        sw = list(grads)
        sw[i] = torch.cat([_swap_blocks(grads[i][0])[None], grads[i][1:]])
        assert name in _fails(bwd, attn["bwd"], tuple(sw), f"{name} blocks swapped")[0][0]
    sw = list(grads)
    sw[3] = grads[3].flip(0)                                                # its bound has 2e-2 max |ref|: 2^-5 on a column is inside it
    assert "grad_weight" in _fails(bwd, attn["bwd"], tuple(sw), "grad_weight heads reversed")[0][0]
    sw = list(grads)
    sw[4] = grads[4].flip(0)
    assert "grad_bias" in _fails(bwd, attn["bwd"], tuple(sw), "grad_bias heads reversed")[0][0]
    flat = dict(attn["bwd"], proj_weight=attn["bwd"]["proj_weight"] * 0, proj_bias=attn["bwd"]["proj_bias"] * 0)
    labels = " ".join(w for w, _, _ in _fails(bwd, flat, grads, "every pair at the ReLU kink"))     # the allowance cannot excuse it
    assert "kink_pair_share" in labels and "kink_complete_rows" in labels
    nomask = dict(attn["bwd"], mask=None)                                   # the mask ignored by the reference's caller: all differ
    assert _fails(bwd, nomask, grads, "mask dropped")


# ----------------------------------------------------------------------------------------------------------------- MSDA
@pytest.fixture(scope="module")
def msda():
    g = torch.Generator().manual_seed(4)
    levels = [(9, 7), (5, 4)]
    B, H, D, L, P = 2, 8, 32, 2, 4
    S = sum(h * w for h, w in levels)
    shapes = torch.tensor(levels, dtype=torch.int64)
    start = torch.tensor([0, levels[0][0] * levels[0][1]], dtype=torch.int64)
    mask = torch.zeros(B, S, dtype=torch.bool)                              # image 1: right and bottom padding on both levels
    off = 0
    for h, w in levels:
        m = torch.zeros(h, w, dtype=torch.bool)
        m[:, w - 2:] = True
        m[h - 1:, :] = True
        mask[1, off:off + h * w] = m.flatten()
        off += h * w
    value_hm = _rand(g, B, H, S, D)
    value_hm = value_hm.masked_fill(mask[:, None, :, None], 0)              # what value_to_head_major hands on
    offsets = _rand(g, B, S, H, L, P, 2, scale=1.5)
    logits = _rand(g, B, S, H, L * P)
    ref = torch.rand(B, S, L, 2, generator=g) * 0.9 + 0.05
    go = _rand(g, B, S, H * D)
    v = value_hm.permute(0, 2, 1, 3).float().requires_grad_(True)
    o, lg, rp = offsets.float().requires_grad_(True), logits.float().requires_grad_(True), ref.clone().requires_grad_(True)
    loc = torch_ref.sampling_locations_from_reference(rp, o, shapes.float(), P)
    out = torch_ref.msda_core(v, shapes, loc, lg.softmax(-1).view(B, S, H, L, P))
    out.backward(go.float())
    gv_hm = v.grad.permute(0, 2, 1, 3).contiguous()                         # fp32 [B, 8, S, 32]
    args = dict(value_hm=value_hm, spatial_shapes=shapes, level_start_index=start, sampling_offsets=offsets, attn_logits=logits,
                reference_points=ref, grad_output=go, deterministic=None, need_ref_grad=True, grad_producer_out=None)
    return dict(args=args, res=[gv_hm, o.grad.to(BF), lg.grad.to(BF), rp.grad], mask=mask)


def test_msda_checkers(msda):
    hm, relayout = "msda_train_hm.ms_deform_attn_backward_fused_hm", "msda_train_hm.grad_value_from_head_major"
    args, res, mask = msda["args"], msda["res"], msda["mask"]
    _passes(hm, args, res)
    _passes(hm, dict(args, need_ref_grad=False), res[:3] + [None])
    gv = res[0]
    assert "grad_value" in _fails(hm, args, [_scale_column(gv), *res[1:]], "grad_value column scaled")[0][0]
    assert "grad_value" in _fails(hm, args, [gv.flip(1), *res[1:]], "grad_value heads reversed")[0][0]
    sw = torch.cat([_swap_blocks(gv[:, :, :, :].reshape(-1, 32)).reshape(gv.shape)])
    assert "grad_value" in _fails(hm, args, [sw, *res[1:]], "grad_value rows swapped")[0][0]
    assert "grad_logits" in _fails(hm, args, [gv, res[1], _scale_column(res[2], 1), res[3]], "grad_logits column scaled")[0][0]
    assert "grad_offsets" in _fails(hm, args, [gv, _swap_blocks(res[1].reshape(-1, 128)).reshape(res[1].shape), res[2], res[3]],
                                    "grad_offsets rows swapped")[0][0]

    B, _, S, _ = gv.shape
    want = gv.permute(0, 2, 1, 3).reshape(B, S, 256).to(BF)
    assert (want[mask] != 0).any()                                          # padded rows do collect a gradient before the fill
    a = dict(grad_hm=gv, key_padding_mask=mask, out=None)
    _passes(relayout, a, want.masked_fill(mask[..., None], 0))
    _passes(relayout, dict(a, key_padding_mask=None), want)
    _fails(relayout, a, want, "the mask ignored")
    _fails(relayout, a, _swap_blocks(want.masked_fill(mask[..., None], 0)), "rows swapped")
    low = want.masked_fill(mask[..., None], 0).clone()
    low.view(torch.int16)[0, 0, 0] ^= 1                                     # one bit of one element
    _fails(relayout, a, low, "one ulp in one element")
