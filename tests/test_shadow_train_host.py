"""CPU test of the shadow checkers of the training entries outside ops.py (tests/shadow.py, TRAIN_ENTRIES).  Needs neither a GPU
nor the built library: each entry's result is formed by the unfused torch sequence from bf16 (LayerNorm: fp32 too) tensors, in
fp32 arithmetic, rounded where the kernel stores.  Every Cmp of the checker must pass on that -- the float64 reference alone
stays inside its own bounds at these shapes -- and each corruption below must fail it.

The second half does the same for the checkers of a detector step (amp_train, neck, denoising, criterion, optim): the module's own
fp32 torch route as the "kernel", then one planted defect each.

Shapes: FFN 37 rows x F = 64; LayerNorm 5 and 300 rows; attention B = 2, N = M = 37 with a block mask and one fully masked row;
MSDA levels [(9, 7), (5, 4)], B = 2, one padded image.

The last part does it for the entries in front of the neck (backbones.epilogue, frontend.images): fp32 torch operators and the
float64 value rounded once to bf16 as the epilogue kernels, ``ImagePreprocessor.batch_torch`` as the front end; planes of 5 x 7
(35 elements, off the 16-byte grid), channels-last with C = 12 (no multiple of 8), and the uint8 images of the GPU cases themselves,
whose near-tie share is asserted here so that the GPU test cannot be ill-posed by its inputs.
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
    # the log-sum-exp bound carries the scale of the projection (shadow.boxes_lse_bound): twice a row's bound fails, half of it passes
    room = shadow.boxes_lse_bound(attn["fwd"]["proj_weight"], 8, lse2.shape[0]).float()
    assert 1e-3 < float(room.min()) and float(room.max()) < 1e-3 + 2.0 ** -9 * 64 * float(attn["fwd"]["proj_weight"].abs().max()) + 1e-12
    assert "lse" in _fails(fwd, attn["fwd"], (out, lse2 + 2 * room / math.log(2.0)), "lse shifted by twice its bound")[0][0]
    _passes(fwd, attn["fwd"], (out, lse2 + 0.5 * room / math.log(2.0)))
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


@pytest.mark.parametrize("junk", [math.nan, math.inf, -math.inf])
def test_excluded_element_may_be_inaccurate_but_not_unwritten(junk):
    """`keep` takes an element out of the comparison (a kink point of grad_loc): any finite value passes there, a NaN or inf the
    reference lacks does not."""
    ref, keep = torch.tensor([1.0, 2.0, 3.0, math.inf]), torch.tensor([True, False, True, False])
    got = ref.clone()
    got[1] = 1e9                                                            # excluded and finite: not looked at
    assert shadow._compare(shadow.Cmp("x", got, ref, 1e-6, keep))[:3] == (0.0, 0, 2)
    assert shadow._compare(shadow.Cmp("x", got, ref.nan_to_num(posinf=7.0), 1e-6, keep))[:2] == (math.inf, 1)   # inf the reference lacks
    got[1] = junk
    worst, failing, checked, where = shadow._compare(shadow.Cmp("x", got, ref, 1e-6, keep))
    assert (worst, failing, checked) == (math.inf, 1, 2) and where.startswith("x[1]")
    both = torch.tensor([math.nan, math.nan, 3.0, math.inf])                # NaN on both sides stays equal, kept or not
    assert shadow._compare(shadow.Cmp("x", both.clone(), both, 1e-6, keep))[:2] == (0.0, 0)


# ====================================================================================== the detector step's checkers
# amp_train, neck, denoising, criterion, optim: the "kernel result" is the module's own fp32 torch route on the same operands (the
# checker's e32 yardstick is that route's error, so it passes by construction and by no wider margin than the bound's factor 4); then
# one planted defect each, of the kind a kernel can have.
F32, F64 = torch.float32, torch.float64


def _cmp(key, args, res, label):
    with torch.no_grad():
        return next(c for c in shadow.TRAIN_ENTRIES[key](args, res) if c.label == label)


def _bump(key, args, res, label, tensor, idx, factor=4.0):
    """`tensor` (the part of `res` that Cmp `label` compares) with element `idx` moved `factor` times its bound off the reference."""
    c = _cmp(key, args, res, label)
    bound = c.bound[idx] if torch.is_tensor(c.bound) else c.bound
    out = tensor.clone()
    out[idx] = (c.ref[idx].double() + factor * float(bound)).to(out.dtype)
    return out


def _labels(bad):
    return " ".join(w for w, _, _ in bad)


def test_new_entries_are_all_exercised_here():
    new = {k for k in shadow.TRAIN_ENTRIES if k.split(".")[0] in ("amp_train", "neck", "denoising", "criterion", "optim", "backbones", "frontend")}
    assert new == set(DETECTOR_CASES), (sorted(new - set(DETECTOR_CASES)), sorted(set(DETECTOR_CASES) - new))


DETECTOR_CASES = {}


def _case(key):
    def register(fn):
        DETECTOR_CASES[key] = fn
        return fn
    return register


# ------------------------------------------------------------------------------------------------- mixed LayerNorm / FFN
@_case("amp_train.add_layer_norm_mixed_train")
def test_mixed_layer_norm_forward():
    key = "amp_train.add_layer_norm_mixed_train"
    x, r, w, b, _ = _ln_case(BF, 37, True)
    r, w, b = r.float() * 1.01, w.float(), b.float()                         # bf16 x, fp32 residual and parameters
    s = x.float() + r
    out = torch.nn.functional.layer_norm(s, (256,), w, b, 1e-5)
    stats = torch.stack([s.mean(-1), (s.var(-1, unbiased=False) + 1e-5).rsqrt()], -1)
    a = dict(x=x, residual=r, weight=w, bias=b, eps=1e-5)
    _passes(key, a, (out, stats))
    assert "out[11, 5]" in _labels(_fails(key, a, (_bump(key, a, (out, stats), "out", out, (11, 5)), stats), "one element 4 x its bound off"))
    alone = torch.nn.functional.layer_norm(x.float(), (256,), w, b, 1e-5)
    assert "out" in _labels(_fails(key, a, (alone, stats), "the residual not added"))
    bumped = stats.clone()
    bumped[20, 1] *= 1 + 2.0 ** -14
    assert "rstd[20]" in _labels(_fails(key, a, (out, bumped), "one rstd off by 2^-14"))


@_case("amp_train.add_layer_norm_mixed_backward")
def test_mixed_layer_norm_backward():
    key = "amp_train.add_layer_norm_mixed_backward"
    x, r, w, b, dy = _ln_case(BF, 300, True)
    r, w, dy = r.float() * 1.01, w.float(), dy.float()
    s = (x.float() + r).requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    bfl = b.float().requires_grad_(True)
    torch.nn.functional.layer_norm(s, (256,), wf, bfl, 1e-5).backward(dy)
    dx, dg, db = s.grad, wf.grad, bfl.grad
    stats = torch.zeros(300, 2)
    a = dict(dy=dy, x=x, residual=r, stats=stats, weight=w, need_params=True)
    res = (dx, dx.to(BF), dg, db)
    _passes(key, a, res)
    _passes(key, dict(a, need_params=False), (dx, dx.to(BF), None, None))
    _passes(key, dict(a, residual=None, x=(x.float() + r).to(BF)), (None,) + _mixed_ln_bf16_only(x, r, w, dy))
    assert "dx[7, 9]" in _labels(_fails(key, a, (_bump(key, a, res, "dx", dx, (7, 9)), dx.to(BF), dg, db), "dx element 4 x its bound off"))
    low = dx.to(BF)
    low.view(torch.int16)[3, 3] ^= 1
    assert "dx_bf16[3, 3]" in _labels(_fails(key, a, (dx, low, dg, db), "the bf16 dx one ulp from the rounding of the fp32 dx"))
    big = int(dg.abs().argmax())
    assert f"dgamma[{big}]" in _labels(_fails(key, a, (dx, dx.to(BF), _bump(key, a, res, "dgamma", dg, (big,)), db), "dgamma 4 x its bound off"))


def _mixed_ln_bf16_only(x, r, w, dy):
    xb = (x.float() + r).to(BF)
    s = xb.float().requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    bfl = torch.zeros(256, requires_grad=True)
    torch.nn.functional.layer_norm(s, (256,), wf, bfl, 1e-5).backward(dy)
    return s.grad.to(BF), wf.grad, bfl.grad


@pytest.fixture(scope="module")
def ffn32(ffn):
    """The bf16 fixture's operands as fp32 tensors that are NOT bf16 values (the kernel rounds them), results from the rounded ones."""
    g = torch.Generator().manual_seed(8)
    jitter = lambda t: t.float() * (1 + 2.0 ** -8 * torch.rand(t.shape, generator=g))                  # noqa: E731
    x, w1, b1, w2, b2 = (jitter(ffn["fwd"][k]) for k in ("x", "w1", "b1", "w2", "b2"))
    rb = lambda t: t.to(BF).float()                                                                      # noqa: E731
    hid = torch.relu(rb(x) @ rb(w1).t() + rb(b1)).to(BF)
    out = (hid.float() @ rb(w2).t() + rb(b2)).to(BF)
    dy = ffn["bwd"]["dy"].float()
    dh = (dy.to(BF).float() @ rb(w2)).to(BF) * (hid > 0)
    dx = dh.float() @ rb(w1)
    return dict(fwd=dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2), bwd=dict(dy=dy, hid=hid, w1=w1, w2=w2, fp32_dx=True), out=out, hid=hid, dh=dh, dx=dx)


@_case("amp_train.ffn_mixed_train")
def test_mixed_ffn_forward(ffn32):
    key, c = "amp_train.ffn_mixed_train", ffn32
    xlp = c["fwd"]["x"].to(BF)
    assert not torch.equal(xlp.float(), c["fwd"]["x"])
    _passes(key, c["fwd"], (c["out"], c["hid"], xlp))
    assert "out" in _labels(_fails(key, c["fwd"], (_scale_column(c["out"]), c["hid"], xlp), "out column scaled"))
    assert "hid" in _labels(_fails(key, c["fwd"], (c["out"], _swap_blocks(c["hid"]), xlp), "hid blocks swapped"))
    trunc = (c["fwd"]["x"].view(torch.int32) & -65536).view(F32).to(BF)                                # truncated, not rounded to nearest
    assert not torch.equal(trunc, xlp)
    assert "x_bf16" in _labels(_fails(key, c["fwd"], (c["out"], c["hid"], trunc), "x truncated instead of rounded"))


@_case("amp_train.ffn_mixed_backward")
def test_mixed_ffn_backward(ffn32):
    key, c = "amp_train.ffn_mixed_backward", ffn32
    res = (c["dx"], c["dh"])
    _passes(key, c["bwd"], res)
    _passes(key, dict(c["bwd"], fp32_dx=False), (c["dx"].to(BF), c["dh"]))
    assert "dx[5, 17]" in _labels(_fails(key, c["bwd"], (_bump(key, c["bwd"], res, "dx", c["dx"], (5, 17)), c["dh"]), "dx 4 x its bound off"))
    assert "dx" in _labels(_fails(key, c["bwd"], (c["dx"].to(BF).float(), c["dh"]), "the fp32 dx rounded to bf16 on the way"))
    unrounded = c["dh"].float() @ c["bwd"]["w1"]                            # dx from the fp32 w1 instead of its bf16 rounding
    assert "dx" in _labels(_fails(key, c["bwd"], (unrounded, c["dh"]), "w1 not rounded"))


# ------------------------------------------------------------------------------------------------------------------ neck
GN_LEVELS = ((9, 7), (5, 4), (1, 2))


@pytest.fixture(scope="module")
def gn():
    g = torch.Generator().manual_seed(12)
    B, C, G = 2, 32, 8
    xs = [torch.randn(B, C, h, w, generator=g) + 0.3 for h, w in GN_LEVELS]
    ws = [1.0 + 0.3 * torch.randn(C, generator=g) for _ in GN_LEVELS]
    bs = [0.3 * torch.randn(C, generator=g) for _ in GN_LEVELS]
    gos = [torch.randn(B, C, h, w, generator=g) for h, w in GN_LEVELS]

    def run(groups):
        out = []
        for x, w, b, go in zip(xs, ws, bs, gos):
            x, w, b = (t.clone().requires_grad_() for t in (x, w, b))
            y = torch.nn.functional.group_norm(x, groups, w, b, 1e-5)
            y.backward(go)
            out.append((y.detach(), x.grad, w.grad, b.grad))
        return out

    def stats(groups):
        flat = [x.reshape(B, groups, -1) for x in xs]
        return torch.stack([f.mean(-1) for f in flat]), torch.stack([(f.var(-1, unbiased=False) + 1e-5).rsqrt() for f in flat])
    return dict(G=G, xs=xs, ws=ws, bs=bs, gos=gos, run=run, stats=stats)


@_case("neck.group_norm_levels_forward")
def test_group_norm_forward_checker(gn):
    key = "neck.group_norm_levels_forward"
    a = dict(xs=gn["xs"], weights=gn["ws"], biases=gn["bs"], num_groups=gn["G"], eps=1e-5)
    ys = [r[0] for r in gn["run"](gn["G"])]
    mean, rstd = gn["stats"](gn["G"])
    _passes(key, a, (ys, mean, rstd))
    y1 = _bump(key, a, (ys, mean, rstd), "y1", ys[1], (1, 17, 2, 3))
    assert "y1[1, 17, 2, 3]" in _labels(_fails(key, a, ([ys[0], y1, ys[2]], mean, rstd), "one element 4 x its bound off"))
    wrong = torch.stack([(x.reshape(2, 4, -1).var(-1, unbiased=False) + 1e-5).rsqrt().repeat_interleave(2, 1) for x in gn["xs"]])
    assert wrong.shape == rstd.shape
    assert "rstd" in _labels(_fails(key, a, (ys, mean, wrong), "rstd taken with the wrong group size"))
    assert "y0" in _labels(_fails(key, a, ([r[0] for r in gn["run"](4)], mean, rstd), "normalised over the wrong group size"))
    swapped = [torch.nn.functional.group_norm(x, gn["G"], gn["ws"][(l + 1) % 3], gn["bs"][l], 1e-5) for l, x in enumerate(gn["xs"])]
    assert "y0" in _labels(_fails(key, a, (swapped, mean, rstd), "another level's weight"))


@_case("neck.group_norm_levels_backward")
def test_group_norm_backward_checker(gn):
    key = "neck.group_norm_levels_backward"
    mean, rstd = gn["stats"](gn["G"])
    a = dict(grads=gn["gos"], xs=gn["xs"], weights=gn["ws"], mean=mean, rstd=rstd, num_groups=gn["G"])
    pack = lambda rows: ([r[1] for r in rows], torch.stack([r[2] for r in rows]), torch.stack([r[3] for r in rows]))    # noqa: E731
    res = pack(gn["run"](gn["G"]))
    _passes(key, a, res)
    wrong = pack(gn["run"](4))                                              # the backward of statistics over groups twice the size
    assert "dx0" in _labels(_fails(key, a, (wrong[0], res[1], res[2]), "rstd taken with the wrong group size"))
    dg = _bump(key, a, res, "dgamma1", res[1][1], (13,))
    dgamma = res[1].clone()
    dgamma[1] = dg
    assert "dgamma1[13]" in _labels(_fails(key, a, (res[0], dgamma, res[2]), "dgamma element 4 x its bound off"))
    assert "dbeta" in _labels(_fails(key, a, (res[0], res[1], res[2].flip(0)), "dbeta levels reversed"))


def _pyramid_mask():
    m = torch.ones(2, 37, 53, dtype=torch.bool)
    m[0, :, :] = False
    m[1, :20, :31] = False
    return m, [(10, 14), (5, 7), (3, 4)]


@_case("neck._masks_and_counts")
def test_masks_and_counts_checker():
    key = "neck._masks_and_counts"
    mask, level_hw = _pyramid_mask()
    masks, ys, xs = shadow._cpu_masks(mask, level_hw)
    cum = torch.cat([t.reshape(-1) for t in (*ys, *xs)])
    a = dict(mask=mask, level_hw=level_hw)
    _passes(key, a, (masks, cum))
    _passes(key, dict(a, mask=mask.float() * 3.0), (masks, cum))
    off = cum.clone()
    off[200] += 1
    assert "counts[200]" in _labels(_fails(key, a, (masks, off), "one running count off by one"))
    flipped = [m.clone() for m in masks]
    flipped[1][1, 2, 4] ^= True
    assert "mask1[1, 2, 4]" in _labels(_fails(key, a, (flipped, cum), "one mask pixel flipped"))
    assert "counts" in _labels(_fails(key, a, (masks, torch.cat([t.reshape(-1) for t in (*xs, *ys)])), "the two count halves exchanged"))


@_case("neck._sine_pos_packed")
@pytest.mark.parametrize("normalize,offset", [(True, -0.5), (False, 0.0)])
def test_sine_pos_checker(normalize, offset):
    from relation_detr_amd.neck import PositionEmbeddingSine, sine_dim_t
    key = "neck._sine_pos_packed"
    mask, level_hw = _pyramid_mask()
    masks, ys, xs = shadow._cpu_masks(mask, level_hw)
    cum = torch.cat([t.reshape(-1) for t in (*ys, *xs)])
    pe = PositionEmbeddingSine(16, 10000, normalize, offset=offset, fused=False)
    pos = [pe.forward_torch(m) for m in masks]
    a = dict(cum=cum, B=2, level_hw=level_hw, dim_t=sine_dim_t(16, 10000), num_pos_feats=16, normalize=normalize, scale=pe.scale, eps=pe.eps,
             offset=offset, dtype=F32)
    _passes(key, a, pos)
    _passes(key, dict(a, dtype=BF), [p.to(BF) for p in pos])
    p1 = _bump(key, a, pos, "pos1", pos[1], (1, 20, 2, 3))
    assert "pos1[1, 20, 2, 3]" in _labels(_fails(key, a, [pos[0], p1, pos[2]], "one element 4 x its bound off"))
    assert "pos0" in _labels(_fails(key, a, [torch.cat((p[:, 16:], p[:, :16]), 1) for p in pos], "the y and x halves exchanged"))


# ------------------------------------------------------------------------------------------------------------- denoising
DN_C = 7


@pytest.fixture(scope="module")
def cdn():
    from relation_detr_amd import denoising as dn
    g = torch.Generator().manual_seed(21)
    counts, groups = [3, 0, 5], 2
    G = sum(counts)
    labels = torch.randint(0, DN_C, (G,), generator=g)
    boxes = torch.cat((0.05 + 0.9 * torch.rand(G, 2, generator=g), 0.02 + 0.5 * torch.rand(G, 2, generator=g)), -1)
    embed = torch.randn(DN_C, 64, generator=g)
    key = 0xC0FFEE
    noise = dn.cdn_noise(key, 2 * groups * G, DN_C, "cpu")
    args = dict(embed=embed, gt_labels=labels, gt_boxes=boxes, counts=counts, groups=groups, label_noise_prob=0.6, box_noise_scale=1.0,
                noise=noise, key=None)
    res = dn._cdn_queries_torch(embed, labels, boxes, counts, groups, 0.6, 1.0, noise)
    return dict(dn=dn, args=args, res=res, key=key, Q=2 * groups * G)


@_case("denoising.cdn_noise")
def test_cdn_noise_checker(cdn):
    key, dn = "denoising.cdn_noise", cdn["dn"]
    a = dict(key=cdn["key"], Q=cdn["Q"], num_classes=DN_C, device="cuda:0")
    assert shadow.TRAIN_ENTRIES[key].applies(a) and not shadow.TRAIN_ENTRIES[key].applies(dict(a, device="cpu"))
    draws = dn.cdn_noise(cdn["key"], cdn["Q"], DN_C, "cpu")
    _passes(key, a, draws)
    shifted = dn.cdn_noise(cdn["key"], cdn["Q"] + 1, DN_C, "cpu")            # row r holds the draw of counter r + 1
    assert "box_u" in _labels(_fails(key, a, (draws[0], draws[1], draws[2], shifted[3][1:]), "one draw shifted by one counter"))
    assert "label_r" in _labels(_fails(key, a, dn.cdn_noise(cdn["key"] + 1, cdn["Q"], DN_C, "cpu"), "another key"))


@_case("denoising.denoising_mask")
def test_denoising_mask_checker(cdn):
    key, dn = "denoising.denoising_mask", cdn["dn"]
    a = dict(groups=2, group_size=10, num_queries=9, device="cuda:0", fused=True)
    entry = shadow.TRAIN_ENTRIES[key]
    assert entry.applies(a) and not entry.applies(dict(a, fused=False)) and not entry.applies(dict(a, device="cpu"))
    mask = dn.denoising_mask(2, 10, 9, "cpu", fused=False)
    _passes(key, a, mask)
    seen = mask.clone()
    seen[3, 14] = False                                                       # a denoising query sees another group
    assert "mask[3, 14]" in _labels(_fails(key, a, seen, "one pair visible across groups"))


@_case("denoising.cdn_queries_forward")
def test_cdn_queries_checker(cdn):
    key, dn, a, res = "denoising.cdn_queries_forward", cdn["dn"], cdn["args"], cdn["res"]
    _passes(key, a, res)
    _passes(key, dict(a, noise=None, key=cdn["key"]), res)                   # the keyed call: the checker rebuilds the draws
    box = _bump(key, a, res, "box_query", res[1], (2, 13, 1))
    assert "box_query[2, 13, 1]" in _labels(_fails(key, a, (res[0], box, res[2]), "one box element 4 x its bound off"))
    shifted = dn.cdn_noise(cdn["key"], cdn["Q"] + 1, DN_C, "cpu")
    other = dn._cdn_queries_torch(a["embed"], a["gt_labels"], a["gt_boxes"], a["counts"], a["groups"], 0.6, 1.0,
                                  (a["noise"][0], a["noise"][1], a["noise"][2], shifted[3][1:]))
    assert "box_query" in _labels(_fails(key, a, other, "one noise draw shifted by one counter"))
    pad = res[0].clone()
    assert (res[2][1] < 0).all()
    pad[1, 0, 0] = 1.0                                                        # image 1 has no box: its slots are padding, exactly 0
    assert "label_query[1, 0, 0]" in _labels(_fails(key, a, (pad, res[1], res[2]), "a padded slot not zero"))


@_case("denoising.cdn_embed_backward")
def test_cdn_embed_backward_checker(cdn):
    key = "denoising.cdn_embed_backward"
    noised = cdn["res"][2]
    grad = torch.randn(*noised.shape, 64, generator=torch.Generator().manual_seed(2))
    used = noised >= 0
    want = torch.zeros(DN_C, 64).index_add_(0, noised[used].long(), grad[used])
    a = dict(grad_label_query=grad, noised_label=noised, num_classes=DN_C)
    _passes(key, a, want)
    _passes(key, dict(a, grad_label_query=grad.to(BF)), torch.zeros(DN_C, 64).index_add_(0, noised[used].long(), grad.to(BF)[used].float()).to(BF))
    assert "grad_embed[3, 5]" in _labels(_fails(key, a, _bump(key, a, want, "grad_embed", want, (3, 5)), "one element 4 x its bound off"))
    padded = torch.zeros(DN_C, 64).index_add_(0, noised.clamp(min=0).flatten().long(), grad.reshape(-1, 64))
    assert "grad_embed[0" in _labels(_fails(key, a, padded, "the padded slots summed into class 0"))


# ------------------------------------------------------------------------------------------------------------- criterion
@pytest.fixture(scope="module")
def crit_case():
    from relation_detr_amd import criterion as crit
    g = torch.Generator().manual_seed(31)
    R, N, C, counts = 4, 23, 7, [3, 5]
    B, Gmax = 2, 5
    logits = (2 * torch.randn(R, N, C, generator=g)).clamp(-6, 6)
    boxes = torch.cat((torch.rand(R, N, 2, generator=g), 0.02 + 0.4 * torch.rand(R, N, 2, generator=g)), -1)
    gt_boxes = torch.cat((torch.rand(B, Gmax, 2, generator=g), 0.02 + 0.4 * torch.rand(B, Gmax, 2, generator=g)), -1)
    gt_labels = torch.randint(0, C, (B, Gmax), generator=g, dtype=torch.int32)
    gt_count = torch.tensor(counts, dtype=torch.int32)
    cost_args = dict(logits=logits, boxes=boxes, gt_boxes=gt_boxes, gt_labels=gt_labels, gt_count=gt_count, cost_class=2.0, cost_bbox=5.0,
                     cost_giou=2.0, alpha=0.25, gamma=2.0, fused=True, out=None)
    cost = crit.match_cost(logits, boxes, gt_boxes, gt_labels, gt_count, fused=False)
    return dict(crit=crit, cost_args=cost_args, cost=cost, counts=counts, R=R, N=N, C=C)


@_case("criterion.match_cost")
def test_match_cost_checker(crit_case):
    key, c = "criterion.match_cost", crit_case
    a, cost = c["cost_args"], c["cost"]
    assert not shadow.TRAIN_ENTRIES[key].applies(a) and not shadow.TRAIN_ENTRIES[key].applies(dict(a, fused=False))      # CPU tensors
    _passes(key, a, cost)
    _passes(key, dict(a, logits=a["logits"].to(BF)), c["crit"].match_cost(a["logits"].to(BF), a["boxes"], a["gt_boxes"], a["gt_labels"],
                                                                           a["gt_count"], fused=False))
    assert "cost[2, 9, 1]" in _labels(_fails(key, a, _bump(key, a, cost, "cost", cost, (2, 9, 1)), "one element 4 x its bound off"))
    dirty = cost.clone()
    dirty[0, 4, 3] = 2.0 ** -30                                               # image 0 has 3 boxes: column 3 is padding
    bad = _fails(key, a, dirty, "a padded cost column not zero")
    assert len(bad) == 1 and "padded_columns[0, 4, 3]" in bad[0][0]
    wrong_image = cost.clone()
    wrong_image[1], wrong_image[3] = cost[3], cost[1]
    assert "cost" in _labels(_fails(key, a, wrong_image.roll(1, 0), "rows against the other image's targets"))


@_case("criterion.set_loss_forward")
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_set_loss_checker(crit_case, dtype):
    key, c = "criterion.set_loss_forward", crit_case
    g = torch.Generator().manual_seed(41)
    ca = c["cost_args"]
    match = torch.full((c["R"], c["N"]), -1, dtype=torch.int32)
    for r in range(c["R"]):
        match[r] = torch.randint(-1, c["counts"][r % 2], (c["N"],), generator=g, dtype=torch.int32)
    a = dict(logits=ca["logits"].to(dtype), boxes=ca["boxes"], match=match, gt_boxes=ca["gt_boxes"], gt_labels=ca["gt_labels"], n_split=6,
             inv_norm_a=1.0 / 12.0, inv_norm_b=1.0 / 5.0, alpha=0.25, gamma=2.0)
    sums, dlogits, dl1, dgiou = shadow._set_loss_route(a, F32)
    res = (sums, dlogits.to(dtype), dl1, dgiou)
    _passes(key, a, res)
    dl = _bump(key, a, res, "dlogits", res[1], (1, 8, 2), factor=4.0 if dtype == F32 else 8.0)
    assert "dlogits[1, 8, 2]" in _labels(_fails(key, a, (sums, dl, dl1, dgiou), "one dlogits element off"))
    other = shadow._set_loss_route(dict(a, n_split=7), F32)
    assert not torch.equal(other[0], sums)
    bad = _labels(_fails(key, a, (other[0], other[1].to(dtype), other[2], other[3]), "n_split off by one"))
    assert "sums" in bad or "dlogits" in bad
    assert "dbox_giou" in _labels(_fails(key, a, (sums, res[1], dl1, dl1), "the L1 gradient in the GIoU gradient's place"))
    unscaled = shadow._set_loss_route(dict(a, inv_norm_a=1.0), F32)
    assert "sums" in _labels(_fails(key, a, (unscaled[0], res[1], dl1, dgiou), "the denoising segment not normalised"))


@_case("criterion.assign_match")
def test_assign_match_checker(crit_case):
    key, c = "criterion.assign_match", crit_case
    crit, cost, counts = c["crit"], c["cost"], c["counts"]
    entry = shadow.TRAIN_ENTRIES[key]
    for repeat, skip, dn_meta in ((1, 0, None), (6, 0, None), (1, 10, (1, 10)), (1, 10, (2, 5))):
        a = dict(cost=cost, gt_count=torch.tensor(counts, dtype=torch.int32), repeat=repeat, skip=skip, dn_meta=dn_meta, out=None, fused=True)
        assert not entry.applies(a)                                           # a CPU cost goes to scipy: not a launch, not recorded
        table, status = crit.assign_match(cost, counts, repeat, skip, dn_meta, fused=False)
        _passes(key, a, (table, status))
        m = table.clone()
        row = m[2, skip:]
        q = int((row >= 0).nonzero()[0])
        free = (row < 0).nonzero().flatten() if repeat == 1 else (row != row[q]).nonzero().flatten()
        worse = max(free.tolist(), key=lambda j: float(cost[2, j, row[q]]))
        assert cost[2, worse, row[q]] > cost[2, q, row[q]]
        if repeat == 1:
            row[worse], row[q] = row[q], -1                                   # the target handed to a costlier query: still valid
        else:
            row[worse], row[q] = row[q].clone(), row[worse].clone()           # two queries exchange their targets
        bad = _fails(key, a, (m, status), "one matched pair swapped to a costlier one")
        assert len(bad) == 1 and "total_cost[2]" in bad[0][0], bad
        twice = table.clone()
        t = twice[1, skip:]
        pair = (t >= 0).nonzero().flatten()[:2]
        if repeat == 1:
            t[pair[1]] = t[pair[0]]                                           # one gt matched twice, another never
            assert "valid_assignment[1]" in _labels(_fails(key, a, (twice, status), "a gt matched twice"))
        beyond = table.clone()
        beyond[0, skip + 1] = 4                                               # image 0 has 3 boxes
        assert "valid_assignment[0]" in _labels(_fails(key, a, (beyond, status), "an index at or beyond the image's count"))
        flagged = status.clone()
        flagged[3] = 1
        assert "status[3]" in _labels(_fails(key, a, (table, flagged), "status not 0"))
        if skip:
            prefix = table.clone()
            prefix[1, 4] = -1 if int(prefix[1, 4]) >= 0 else 0
            bad = _fails(key, a, (prefix, status), "a denoising match outside the fixed pattern")
            assert len(bad) == 1 and "denoising_prefix[1]" in bad[0][0], bad


# ------------------------------------------------------------------------------------------------------------- optimizer
def _optimizer(step2):
    """A CPU FusedAdamW over five tensors in two groups -- one without a gradient -- before its first or second step."""
    from relation_detr_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(51)
    params = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 91, 256, 8193, 7)]
    opt = FusedAdamW([{"params": params[:3]}, {"params": params[3:], "lr": 3e-4, "weight_decay": 0.0}], lr=1e-3, weight_decay=1e-2, fused=False)
    for round_ in range(2 if step2 else 1):
        for i, p in enumerate(params):
            p.grad = None if i == 4 else torch.randn(p.shape, generator=g) * (1.0 if i != 1 else 1e-3)
        if round_ == 0 and step2:
            opt.step()
    return opt, params


def _apply_fp32_route(opt, rows, coef, unclipped_v=False, keep_step=False):
    """Write what the fp32 torch route makes of `rows` into `opt` (the "kernel"), with the planted defects on request."""
    from helpers import torch_route_step
    scaled = [dict(r, g=None if r["g"] is None else r["g"] * coef) for r in rows]
    _, out = torch_route_step(opt, scaled, None, F32)
    _, raw = torch_route_step(opt, rows, None, F32)
    i = 0
    with torch.no_grad():
        for group in opt.param_groups:
            for p in group["params"]:
                if rows[i]["g"] is not None:
                    state = opt._init_state(p)
                    p.copy_(out[i][0])
                    state["exp_avg"].copy_(out[i][1])
                    state["exp_avg_sq"].copy_(raw[i][2] if unclipped_v else out[i][2])
                    state["step"] = torch.tensor(rows[i]["step"] + (0.0 if keep_step else 1.0))
                i += 1


@_case("optim.FusedAdamW._clip_fused")
def test_clip_checker():
    from helpers import snapshot, torch_route_step
    key = "optim.FusedAdamW._clip_fused"
    opt, _ = _optimizer(step2=True)
    rows = snapshot(opt)
    norm, _ = torch_route_step(opt, rows, 0.1, F32)
    coef = (0.1 / (norm + 1e-6)).clamp(max=1.0)
    assert coef < 1
    a = dict(self=opt, max_norm=0.1, rows=rows, coef=None)
    opt._armed = torch.stack([norm, coef])
    _passes(key, a, norm)
    assert "total_norm" in _labels(_fails(key, a, norm * (1 + 2.0 ** -18), "the norm 2^-18 off"))
    partial = torch.cat([r["g"].flatten() for r in rows[:3] if r["g"] is not None]).norm()
    assert "total_norm" in _labels(_fails(key, a, partial, "the norm of the first group alone"))
    opt._armed = torch.stack([norm, torch.ones(())])
    assert "coef" in _labels(_fails(key, a, norm, "the coefficient left at 1"))
    opt._armed = None


@_case("optim.FusedAdamW._step_fused")
@pytest.mark.parametrize("step2", [False, True], ids=["first_step", "second_step"])
def test_step_checker(step2):
    from helpers import snapshot
    key = "optim.FusedAdamW._step_fused"
    coef = torch.tensor(0.0371)

    def run(**defect):
        opt, params = _optimizer(step2)
        rows = snapshot(opt)
        assert [r["step"] for r in rows] == ([1.0] * 4 + [0.0] if step2 else [0.0] * 5)
        _apply_fp32_route(opt, rows, coef, **defect)
        return dict(self=opt, rows=rows, coef=coef), params
    a, params = run()
    _passes(key, a, None)
    a, params = run()
    c = _cmp(key, a, None, "param")
    at = 5 + 91 + 100                                                         # flat: the third tensor, element 100
    with torch.no_grad():
        params[2][100] = (c.ref[at] + 4 * c.bound[at]).float()
    bad = _fails(key, a, None, "one parameter element 4 x its bound off")
    assert len(bad) == 1 and f"param[{at}]" in bad[0][0], bad
    a, params = run()
    with torch.no_grad():
        params[4][3] += 2.0 ** -20                                            # the tensor without a gradient keeps its bits
    assert f"param[{5 + 91 + 256 + 8193 + 3}]" in _labels(_fails(key, a, None, "a tensor without a gradient written"))
    a, _ = run(unclipped_v=True)
    bad = _fails(key, a, None, "exp_avg_sq updated with the unclipped gradient")
    assert len(bad) == 1 and "exp_avg_sq" in bad[0][0], bad
    a, _ = run(keep_step=True)
    bad = _fails(key, a, None, "step not advanced")
    assert len(bad) == 1 and "step[0]" in bad[0][0], bad
    a, _ = run()
    a["coef"] = None                                                          # the reference then steps with the unclipped gradients
    assert "exp_avg" in _labels(_fails(key, a, None, "the clip coefficient applied where none was armed"))


# ------------------------------------------------------------------------------------------------- the backbone's epilogues
FWD, BWD, STEM, IMAGES = ("backbones.epilogue.frozen_bn_act_forward", "backbones.epilogue.frozen_bn_act_backward",
                          "backbones.epilogue.stem_bn_relu_maxpool", "frontend.images.batch_images")
POISON = 48.5                                                                    # what 0x42 bytes read as in bf16 (48.56 in fp32)


def _epilogue_case(dtype, channels_last=False, C=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    x, r, dy = (_rand(g, 2, C, 5, 7, dtype=dtype) for _ in range(3))
    if channels_last:
        x, r, dy = (t.contiguous(memory_format=torch.channels_last) for t in (x, r, dy))
    s = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)          # every third channel negative
    return x, r, dy, s, torch.randn(C, generator=g) * 0.5


def _kernel_forward(x, s, h, r, relu):
    """Within the bound by construction: the fp32 operator sequence; for bf16 the float64 value rounded once."""
    from helpers import torch_bn_act
    if x.dtype == F32:
        return torch_bn_act(x, s, h, r, relu)
    return torch_bn_act(x.double(), s.double(), h.double(), None if r is None else r.double(), relu).to(BF)


def _kernel_backward(dy, mask_from, s, relu, want_dres):
    masked = torch.where(mask_from <= 0, torch.zeros_like(dy), dy) if relu else dy
    s4 = s.reshape(1, -1, 1, 1)
    dx = masked * s4 if dy.dtype == F32 else (masked.double() * s4.double()).to(BF)
    return dx, (masked.clone() if want_dres else None)


@_case(FWD)
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_frozen_bn_act_forward_checker(dtype, channels_last):
    x, r, _, s, h = _epilogue_case(dtype, channels_last, C=12)
    for res_in, relu in ((None, True), (r, True), (r, False), (r.float() if dtype == BF else r.to(BF), True)):
        a = dict(x=x, scale=s, shift=h, residual=res_in, relu=relu, out=None)
        used = None if res_in is None else res_in.to(dtype)
        out = _kernel_forward(x, s, h, used, relu)
        _passes(FWD, a, out)
        _passes(FWD, dict(a, out=x.clone()), out)                                 # in place: the wrapper's copy of x is the operand
        c = _cmp(FWD, a, out, "out")
        idx = tuple(int(i) for i in (out.double().abs() == out.double().abs().max()).nonzero()[0])
        bumped = out.clone()
        if dtype == F32:
            bumped[idx] = torch.nextafter(out[idx], out[idx] * 2)                 # exact: one ulp is over
        else:
            bumped[idx] = (c.ref[idx] + 2 * c.bound[idx] * (1 + 2.0 ** -6)).to(BF) + 0
            assert abs(float(bumped[idx]) - float(c.ref[idx])) > float(c.bound[idx])
        bad = _fails(FWD, a, bumped, "one element twice its bound off")
        assert len(bad) == 1 and bad[0][1] == 1, bad
        tail = out.clone()
        tail[1, 4, 4, 4:] = POISON                                          # the last 3 of a plane's 35 elements never written
        bad = _fails(FWD, a, tail, "one plane's tail left at the poison value")
        assert bad[0][1] == 3 and "out[1, 4, 4, " in bad[0][0], bad
        # channel c's constants applied to channel c + 1: what a channels-last kernel does that steps its constants by the wrong phase
        rolled = _kernel_forward(x, s.roll(1), h.roll(1), used, relu)
        assert "out" in _labels(_fails(FWD, a, rolled, "scale and shift of channel c applied to channel c + 1"))
    assert x.is_contiguous(memory_format=torch.channels_last) == channels_last and x.shape[1] % 8


@_case(BWD)
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_frozen_bn_act_backward_checker(dtype):
    x, r, dy, s, h = _epilogue_case(dtype)
    y = _kernel_forward(x, s, h, r, True)
    assert bool(((x <= 0) != (y <= 0)).any())                                      # the two masks differ: a negative scale, a residual
    for relu, want in ((True, True), (True, False), (False, True)):
        a = dict(dy=dy, y=y, scale=s, relu=relu, want_dres=want)
        dx, dres = _kernel_backward(dy, y, s, relu, want)
        _passes(BWD, a, (dx, dres))
        if relu:
            wrong = _kernel_backward(dy, x, s, True, want)
            labels = _labels(_fails(BWD, a, wrong, "the ReLU mask taken from x instead of y"))
            assert "dx" in labels and ("dres[" in labels) == want
            stale = _kernel_backward(dy, torch.ones_like(y), s, True, want)         # a stale saved output: nothing masked
            assert "dx" in _labels(_fails(BWD, a, stale, "no element masked"))
        other = _kernel_backward(dy, y, s, relu, not want)
        bad = _fails(BWD, a, (dx, other[1]), "dres returned where none was asked for" if not want else "no dres where one was asked for")
        assert len(bad) == 1 and "dres_returned" in bad[0][0], bad
        c = _cmp(BWD, a, (dx, dres), "dx")
        idx = tuple(int(i) for i in dx.double().abs().flatten().argmax().reshape(1).new_tensor(
            torch.unravel_index(dx.double().abs().argmax(), dx.shape)))
        bumped = dx.clone()
        if dtype == F32:
            bumped[idx] = torch.nextafter(dx[idx], dx[idx] * 2)
        else:
            bumped[idx] = (c.ref[idx] * (1 + 2 * 2.0 ** -8 * (1 + 2.0 ** -6))).to(BF)
            assert abs(float(bumped[idx]) - float(c.ref[idx])) > float(c.bound[idx])
        bad = _fails(BWD, a, (bumped, dres), "one dx element twice its bound off")
        assert len(bad) == 1 and bad[0][1] == 1 and "dx" in bad[0][0], bad
        if want:
            swapped = _fails(BWD, a, (dres * s.reshape(1, -1, 1, 1).to(dtype), dx), "dres routed to the wrong operand")
            assert "dres[" in _labels(swapped)
            tail = dres.clone()
            tail[0, 2, 4, 4:] = POISON
            assert "dres[0, 2, 4, " in _labels(_fails(BWD, a, (dx, tail), "one plane's tail of dres left at the poison value"))


@_case(STEM)
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_stem_pool_checker(dtype, channels_last):
    from helpers import torch_stem
    g = torch.Generator().manual_seed(5)
    C = 12
    x = _rand(g, 2, C, 9, 13, dtype=dtype)
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x
    s, h = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0), torch.randn(C, generator=g) * 0.5
    kernel = lambda x, s, h: torch_stem(x, s, h) if dtype == F32 else torch_stem(x.double(), s.double(), h.double()).to(BF)   # noqa: E731
    a = dict(x=x, scale=s, shift=h)
    out = kernel(x, s, h)
    assert tuple(out.shape) == (2, C, 5, 7)
    _passes(STEM, a, out)
    c = _cmp(STEM, a, out, "out")
    idx = tuple(int(i) for i in torch.unravel_index(out.double().argmax(), out.shape))
    bumped = out.clone()
    if dtype == F32:
        bumped[idx] = torch.nextafter(out[idx], out[idx] * 2)
    else:
        bumped[idx] = (c.ref[idx] + 2 * c.bound[idx] * (1 + 2.0 ** -6)).to(BF)
        assert abs(float(bumped[idx]) - float(c.ref[idx])) > float(c.bound[idx])
    bad = _fails(STEM, a, bumped, "one pooled element twice its bound off")
    assert len(bad) == 1 and bad[0][1] == 1, bad
    tail = out.clone()
    tail[1, 7, 4, 4:] = POISON
    assert _fails(STEM, a, tail, "one plane's tail left at the poison value")[0][1] == 3
    assert "out" in _labels(_fails(STEM, a, kernel(x, s.roll(1), h.roll(1)), "scale and shift of channel c applied to channel c + 1"))
    # every input negative, scale and shift positive, and so negative that relu gives 0 everywhere: the result is +0.  A kernel that
    # reads the padding as an INPUT of 0 puts relu(0 * s + h) = h into every window at the border
    neg = (-x.float().abs() - 4.0).to(dtype)
    sp, hp = s.abs(), h.abs() + 0.25
    a = dict(x=neg, scale=sp, shift=hp)
    out = kernel(neg, sp, hp)
    assert not out.double().any()
    _passes(STEM, a, out)
    padded = torch.nn.functional.pad(neg.double(), (1, 1, 1, 1))
    leaky = torch.nn.functional.max_pool2d(torch.relu(padded * sp.double().reshape(1, -1, 1, 1) + hp.double().reshape(1, -1, 1, 1)), 3, 2, 0)
    bad = _fails(STEM, a, leaky.to(dtype), "a pooled window that reads the padding as 0")
    assert bad[0][1] == 2 * C * (5 * 7 - 3 * 5), bad                                # every window on the border of the 5 x 7 result


# ------------------------------------------------------------------------------------------------- the image front end
def _front_args(images, pre, **change):
    return dict(dict(images=images, sizes=pre.target_sizes(images), size_divisible=pre.size_divisible, mean=pre.mean, std=pre.std,
                     normalize=not pre.training, dtype=pre.dtype, channels_last=pre.channels_last), **change)


@pytest.fixture(scope="module")
def uint8_batch():
    """The uint8 images of the GPU cases (f), through the torch route."""
    from helpers import DETECTOR_BATCH, DETECTOR_RESIZE, detector_uint8_images
    from relation_detr_amd.frontend import ImagePreprocessor
    images = detector_uint8_images()
    pre = ImagePreprocessor(*DETECTOR_RESIZE, fused=False).eval()
    batch = pre.batch_torch(images)
    assert tuple(batch.tensors.shape) == (3, 3) + DETECTOR_BATCH
    return images, pre, batch


@_case(IMAGES)
def test_batch_images_checker_on_the_gpu_cases_uint8_images(uint8_batch):
    from test_images_host import NEAR_TIE_SHARE
    images, pre, batch = uint8_batch
    a = _front_args(images, pre)
    assert a["sizes"] == [(150, 213), (56, 224), (150, 184)]
    assert 56 * 224 < 0.5 * 160 * 224                                               # the middle image: most of its slot is padding
    _passes(IMAGES, a, batch)
    share = _cmp(IMAGES, a, batch, "near_tie_share")
    valid = sum(3 * oh * ow for oh, ow in a["sizes"])
    print(f"near ties: {int(share.got)} of {valid} valid values, the cap is {NEAR_TIE_SHARE * valid:.0f}")
    assert share.gate and float(share.bound) == NEAR_TIE_SHARE * valid and float(share.got) <= float(share.bound)
    assert NEAR_TIE_SHARE == 0.02
    # bf16 and channels-last: the rounding of the same values
    other = batch._replace(tensors=batch.tensors.to(BF).contiguous(memory_format=torch.channels_last))
    _passes(IMAGES, dict(a, dtype=BF, channels_last=True), other)
    assert "batch_dtype" in _labels(_fails(IMAGES, a, other, "a bf16 batch where fp32 was asked for"))

    def with_tensors(fn):
        t = batch.tensors.clone()
        fn(t)
        return batch._replace(tensors=t)

    def bump(t):
        t[0, 1, 17, 100] = torch.nextafter(t[0, 1, 17, 100], t.new_tensor(10.0))
    bad = _fails(IMAGES, a, with_tensors(bump), "one value one ulp off")
    assert len(bad) == 1 and bad[0][1] == 1 and "image0" in bad[0][0], bad
    shifted = batch._replace(mask=torch.roll(batch.mask, 1, 2))
    assert "mask" in _labels(_fails(IMAGES, a, shifted, "the mask shifted by one pixel"))
    shifted = batch._replace(mask=torch.roll(batch.mask, 1, 1))
    assert "mask" in _labels(_fails(IMAGES, a, shifted, "the mask shifted by one row"))

    def dirty_padding(t):
        t[1, 2, 159, 223] = -0.0                                                   # the padding is +0 to the bit
    bad = _fails(IMAGES, a, with_tensors(dirty_padding), "a padding element that is -0")
    assert len(bad) == 1 and "padding_bits[1, 2, 159, 223]" in bad[0][0], bad

    def poisoned_padding(t):
        t[1, :, 56:, :] = POISON
    assert "padding_bits" in _labels(_fails(IMAGES, a, with_tensors(poisoned_padding), "the padding region not written"))
    swapped = batch._replace(tensors=batch.tensors[[1, 0, 2]], mask=batch.mask[[1, 0, 2]])
    labels = _labels(_fails(IMAGES, a, swapped, "images 0 and 1 in each other's batch slot"))
    assert "mask" in labels and "image0" in labels and "image1" in labels
    values_only = batch._replace(tensors=batch.tensors[[2, 1, 0]])                  # images 0 and 2 have the same height: the values alone
    labels = _labels(_fails(IMAGES, a, values_only, "the values of image 2 in slot 0"))
    assert "image0" in labels and "image2" in labels
    sizes = batch._replace(image_sizes=batch.original_sizes)
    assert "image_sizes" in _labels(_fails(IMAGES, a, sizes, "the original sizes as the resized ones"))
    # too many near ties: the call fails as ill-posed although every value is acceptable
    flat = [torch.full((3, 40, 60), 128, dtype=torch.uint8) for _ in range(2)]
    flat[0][:, ::2] = 127                                                          # rows of 127 and 128: a 2 x downscale lands on 127.5
    a2 = _front_args(flat, pre, sizes=[(20, 60), (40, 60)])
    from relation_detr_amd.frontend import ImagePreprocessor
    res = ImagePreprocessor(fused=False).eval().batch_torch([flat[0][:, :20], flat[1]])       # the layout alone; the gate is what is looked at
    gate = _cmp(IMAGES, a2, res, "near_tie_share")
    assert float(gate.got) > float(gate.bound)


def test_batch_images_checker_float_sources_and_the_copy_path():
    from helpers import detector_float_images
    from relation_detr_amd.frontend import ImagePreprocessor
    from test_images_host import resize64
    images = detector_float_images()
    pre = ImagePreprocessor(150, 224, fused=False).train()                        # training mode: batched only
    batch = pre.batch_torch(images)
    a = _front_args(images, pre)
    assert a["normalize"] is False and a["sizes"] == [(160, 200), (131, 224), (50, 70)] and tuple(batch.tensors.shape) == (3, 3, 160, 224)
    _passes(IMAGES, a, batch)
    t = batch.tensors.clone()
    t[2, 0, 49, 69] = torch.nextafter(t[2, 0, 49, 69], t.new_tensor(10.0))
    bad = _fails(IMAGES, a, batch._replace(tensors=t), "one copied value one ulp off")
    assert len(bad) == 1 and "image2[0, 49, 69]" in bad[0][0], bad
    _passes(IMAGES, dict(a, dtype=BF), batch._replace(tensors=batch.tensors.to(BF)))
    # eval mode, float sources in [0, 1], resized: the float64 filter, normalised, rounded once
    g = torch.Generator().manual_seed(7)
    sources = [torch.rand(3, 45, 70, generator=g), torch.rand(3, 64, 64, generator=g)]
    pre = ImagePreprocessor(fused=False).eval()
    sizes = [(37, 61), (64, 64)]                                                   # one resized, one normalised in place
    a = _front_args(sources, pre, sizes=sizes)
    mean, std = torch.tensor(pre.mean, dtype=F64).view(3, 1, 1), torch.tensor(pre.std, dtype=F64).view(3, 1, 1)
    out = torch.zeros(2, 3, 64, 64)
    out[0, :, :37, :61] = ((torch.from_numpy(resize64(sources[0].numpy(), 37, 61)) - mean) / std).float()
    out[1] = sources[1].clone().sub_(mean.float()).div_(std.float())
    mask = torch.ones(2, 64, 64, dtype=torch.bool)
    mask[0, :37, :61], mask[1] = False, False
    from relation_detr_amd.frontend import ImageBatch
    res = ImageBatch(out, mask, torch.tensor(sizes), torch.tensor([[45, 70], [64, 64]]))
    _passes(IMAGES, a, res)
    _passes(IMAGES, dict(a, dtype=BF), res._replace(tensors=out.to(BF)))
    c = _cmp(IMAGES, a, res, "image0")
    off = out.clone()
    off[0, 1, 5, 9] = (c.ref[1, 5, 9] + 2 * c.bound[1, 5, 9]).float()
    bad = _fails(IMAGES, a, res._replace(tensors=off), "one resized float value twice its bound off")
    assert len(bad) == 1 and bad[0][1] == 1 and "image0[1, 5, 9]" in bad[0][0], bad
    off16 = out.to(BF)
    off16[0, 1, 5, 9] = torch.nextafter(off16[0, 1, 5, 9].float(), torch.tensor(10.0)).to(BF) + 2.0 ** -6
    assert "image0[1, 5, 9]" in _labels(_fails(IMAGES, dict(a, dtype=BF), res._replace(tensors=off16), "one bf16 value two steps off"))


def test_batch_images_checker_applies_where_the_kernel_takes_the_batch(monkeypatch, uint8_batch):
    from relation_detr_amd.frontend import images as fimages
    images, pre, _ = uint8_batch
    applies = shadow.TRAIN_ENTRIES[IMAGES].applies
    a = _front_args(images, pre)
    assert fimages._kernel_takes(images, a["sizes"], 32, True) == "a tensor that is not on a ROCm device" and not applies(a)
    seen = []
    monkeypatch.setattr(fimages, "_kernel_takes", lambda *args: seen.append(args) or None)
    assert applies(a) and applies(dict(a, sizes=None)) and applies(dict(a, images=torch.stack([images[0], images[0]]), sizes=None))
    assert seen[0] == (images, a["sizes"], 32, True) and seen[1][1] == [(211, 300), (100, 400), (333, 410)] and len(seen[2][0]) == 2
    monkeypatch.setattr(fimages, "_kernel_takes", lambda *args: "a downscale beyond 8")
    assert not applies(a)
    assert not applies(dict(a, sizes=a["sizes"][:2])) and not applies(dict(a, dtype=torch.float16))   # batch_images raises before the kernel
