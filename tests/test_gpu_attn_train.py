"""GPU tests of the fused bf16 decoder self-attention training route: the forward with the row log-sum-exp
(csrc/attn.hip, relation_attention_kernel<S, true>), its backward (csrc/attn_bwd.hip), ``ops.relation_attention_train`` /
``ops.relation_attention_backward``, ``ops.RelationAttentionFunction`` and ``RelationSelfAttention`` under ``attn_train_fused``.

Oracle: float64 torch autograd of softmax(Q K^T * scale + bias) V on the same bf16-valued q / k / v, fp32 bias and bf16 dO.
Bounds, per gradient (dq, dk, dv, dbias):
  normwise relative error <= 1.25 x that of the route being replaced (the GEMM + bias-softmax sequence of self_attn.py with
  _BiasSoftmaxFunction, run on the same inputs) + 1e-3;  every element |err| <= 2^-7 |ref| + 2e-2 max|ref|.
"""
import math

import pytest
import torch

from helpers import functional_weights, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, C = 8, 256
SHAPES = [(1, 1, 1), (1, 37, 130), (2, 70, 70), (2, 300, 300), (4, 900, 900), (2, 1100, 1100), (2, 1500, 1500)]
VARIANTS = ["plain", "bias", "mask", "bias_inf_mask"]


@pytest.fixture(scope="module")
def rd():
    import relation_detr_amd
    from relation_detr_amd import _lib
    _lib.load()


def _block_mask(N, M):
    """Denoising-style visibility mask: the first third of the queries and the rest do not see each other (no row fully masked)."""
    nd = N // 3
    if nd == 0 or N != M:
        g = torch.Generator().manual_seed(N * 7 + M)
        m = torch.rand(N, M, generator=g) < 0.2
        m[:, 0] = False
        return m.to(DEV)
    i = torch.arange(N)
    return ((i[:, None] < nd) != (i[None, :] < nd)).to(DEV)


def _inputs(B, N, M, variant, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * N + M)
    if N == M:                                      # q and k as column slices of one packed [B, N, 2C] projection
        qk = torch.randn(B, N, 2 * C, generator=g).to(torch.bfloat16).to(DEV)
        q, k = qk[..., :C], qk[..., C:]
    else:
        q = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(DEV)
        k = torch.randn(B, M, C, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(B, M, C, generator=g).to(torch.bfloat16).to(DEV)
    dout = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(DEV)
    bias = mask = None
    if variant in ("bias", "bias_inf_mask"):
        bias = (torch.rand(B * H, N, M, generator=g) * 3.0).to(DEV)
    if variant == "mask":
        mask = _block_mask(N, M)
    if variant == "bias_inf_mask":
        bias.masked_fill_(_block_mask(N, M), float("-inf"))          # -inf entries, as the decoder's denoising fill
        mask = torch.zeros(N, M, dtype=torch.bool, device=DEV)
        mask[:, M // 2] = M > 1                                        # and one bool-masked key column
    return q, k, v, bias, mask, dout


def _ref64(q, k, v, bias, mask, dout):
    B, N, _ = q.shape
    M, d = k.shape[1], C // H
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    x = qd.view(B, N, H, d).transpose(1, 2) @ kd.view(B, M, H, d).transpose(1, 2).transpose(-1, -2) * d ** -0.5
    bd = None
    if bias is not None:
        bd = bias.detach().double().view(B, H, N, M).requires_grad_(True)
        x = x + bd
    if mask is not None:
        x = x.masked_fill(mask, float("-inf"))
    o = (torch.softmax(x, -1) @ vd.view(B, M, H, d).transpose(1, 2)).transpose(1, 2).reshape(B, N, C)
    o.backward(dout.double())
    lse = torch.logsumexp(x.detach(), -1).reshape(B * H, N)
    return o.detach(), lse, qd.grad, kd.grad, vd.grad, None if bd is None else bd.grad.reshape(B * H, N, M)


def _old_route(q, k, v, bias, mask, dout):
    """The training chain of RelationSelfAttention.forward being replaced (self_attn.py), on the same inputs."""
    from relation_detr_amd.self_attn import _BiasSoftmaxFunction
    B, N, _ = q.shape
    M, d = k.shape[1], C // H
    qo, ko, vo = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    bo = None if bias is None else bias.detach().clone().requires_grad_(True)
    qh = (qo * (1.0 / math.sqrt(d))).view(B, N, H, d).transpose(1, 2).contiguous()
    kh = ko.view(B, M, H, d).transpose(1, 2).contiguous()
    vh = vo.view(B, M, H, d).transpose(1, 2).contiguous()
    scores = torch.matmul(qh, kh.transpose(-1, -2)).float().reshape(B * H, N, M).contiguous()
    probs = _BiasSoftmaxFunction.apply(scores, bo, mask)
    ctx = torch.matmul(probs.view(B, H, N, M).to(vh.dtype), vh).transpose(1, 2).reshape(B, N, C)
    ctx.backward(dout)
    return qo.grad, ko.grad, vo.grad, None if bo is None else bo.grad


def _nrel(got, ref):
    got, ref = got.double(), ref.double()
    den = ref.norm().item()
    return (got - ref).norm().item() / den if den > 0 else (got - ref).norm().item()


def _check_grad(name, got, old, ref, rounding=0.0):
    """`rounding`: for dk and dv, shadow.attention_grad_rounding -- 2^-9 scale |dS|^T |Q| and 2^-9 P^T |dO|, what the bf16 operands
    of the matrix products alone can move them by; where they cancel, max |ref| is no scale for that (tests/shadow.py has the case)."""
    e_new, e_old = _nrel(got, ref), _nrel(old, ref)
    assert e_new <= 1.25 * e_old + 1e-3, (name, e_new, e_old)
    err = (got.double() - ref).abs()
    # 1e-30: the (1, 1, 1) problem has dq = dk = 0 exactly in the reference
    bound = 2.0 ** -7 * ref.abs() + 2e-2 * ref.abs().max() + 1e-30 + rounding
    bad = err > bound
    assert not bad.any(), (name, err.max().item(), int(bad.sum()))


def _grads_and_checks(q, k, v, bias, mask, dout, keep=None):
    from relation_detr_amd import ops
    B, N, _ = q.shape
    out, lse = ops.relation_attention_train(q, k, v, H, bias, mask)
    got = ops.relation_attention_backward(q, k, v, out, lse, dout, H, bias, mask, need_dbias=bias is not None)
    old = _old_route(q, k, v, bias, mask, dout)
    ref = _ref64(q, k, v, bias, mask, dout)[2:]
    import shadow
    with torch.no_grad():
        rounding = shadow._attention_backward64(dict(q=q, k=k, v=v, out=out, dout=dout, num_heads=H, scale=None, mask=mask), bias)[0]["rounding"]
    for name, gn, go, gr in zip(("dq", "dk", "dv", "dbias"), got, old, ref):
        if gr is None:
            assert gn is None
            continue
        extra = rounding.get(name, 0.0)
        if keep is not None:
            gn, go, gr = keep(name, gn), keep(name, go), keep(name, gr)
            extra = keep(name, extra) if name in rounding else extra
        _check_grad(name, gn, go, gr, extra)
    return got


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_train_forward_is_the_inference_kernel_and_lse(rd, B, N, M, variant):
    from relation_detr_amd import ops
    q, k, v, bias, mask, _ = _inputs(B, N, M, variant)
    out, lse = ops.relation_attention_train(q, k, v, H, bias, mask)
    want = ops.relation_attention(q, k, v, H, bias, mask)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))           # bit for bit
    _, lse_ref = _ref64(q, k, v, bias, mask, torch.zeros(B, N, C, dtype=torch.bfloat16, device=DEV))[:2]
    assert lse.shape == (B * H, N) and lse.dtype == torch.float32
    assert (lse.double() - lse_ref).abs().max().item() <= 1e-3


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_backward_matches_float64_and_old_route(rd, B, N, M, variant):
    q, k, v, bias, mask, dout = _inputs(B, N, M, variant)
    _grads_and_checks(q, k, v, bias, mask, dout)


@pytest.mark.parametrize("B,N", [(2, 300), (2, 1100)])
def test_backward_is_deterministic(rd, B, N):
    from relation_detr_amd import ops
    q, k, v, bias, mask, dout = _inputs(B, N, N, "bias_inf_mask", seed=3)
    out, lse = ops.relation_attention_train(q, k, v, H, bias, mask)
    a = ops.relation_attention_backward(q, k, v, out, lse, dout, H, bias, mask, need_dbias=True)
    b = ops.relation_attention_backward(q, k, v, out, lse, dout, H, bias, mask, need_dbias=True)
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                           y.contiguous().view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))


def test_packed_dq_dk_buffer(rd):
    from relation_detr_amd import ops
    q, k, v, bias, mask, dout = _inputs(2, 70, 70, "bias")
    out, lse = ops.relation_attention_train(q, k, v, H, bias, mask)
    dq, dk, dv, db = ops.relation_attention_backward(q, k, v, out, lse, dout, H, bias, mask, need_dbias=True)
    pq, pk, pv, pb = ops.relation_attention_backward(q, k, v, out, lse, dout, H, bias, mask, need_dbias=True, packed_qk=True)
    assert pq.data_ptr() + 2 * C == pk.data_ptr() and pq.stride(1) == 2 * C
    for x, y in ((dq, pq), (dk, pk), (dv, pv), (db, pb)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("B,N", [(2, 70), (2, 300)])
def test_fully_masked_row(rd, B, N):
    from relation_detr_amd import ops
    q, k, v, bias, mask, dout = _inputs(B, N, N, "bias")
    bh_dead, row = 1, 7                                               # image 0, head 1: one row sees no key
    bias[bh_dead, row, :] = float("-inf")
    out, lse = ops.relation_attention_train(q, k, v, H, bias, mask)
    want = ops.relation_attention(q, k, v, H, bias, mask)
    assert torch.equal(torch.isnan(out), torch.isnan(want)) and torch.isnan(out[0, row, 32:64]).all()
    assert torch.isneginf(lse[bh_dead, row])
    torch.cuda.synchronize()
    b0, h0 = divmod(bh_dead, H)

    def keep(name, t):                                                # everything outside the dead (image, head)
        t = t.double()
        if name == "dbias":
            return torch.cat([t[:bh_dead].flatten(), t[bh_dead + 1:].flatten()])
        sel = torch.ones_like(t, dtype=torch.bool)
        sel[b0, :, 32 * h0:32 * h0 + 32] = False
        return t[sel]
    got = _grads_and_checks(q, k, v, bias, mask, dout, keep=keep)
    assert all(bool(torch.isfinite(keep(n, t)).all()) for n, t in zip(("dq", "dk", "dv", "dbias"), got))


def _module_case(N, deferred, on, seed=0):
    from relation_detr_amd import PositionRelationEmbedding, options
    from relation_detr_amd.self_attn import RelationSelfAttention
    torch.manual_seed(0)
    with options.override(attn_train_fused=on):
        mod = RelationSelfAttention(C, H).to(DEV).to(torch.bfloat16).train()
        rel = PositionRelationEmbedding(16, H).to(DEV).to(torch.bfloat16)
    g = torch.Generator().manual_seed(seed + N)
    B = 2
    x = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    pos = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(DEV)
    boxes = torch.cat([torch.rand(B, N, 2, generator=g), torch.rand(B, N, 2, generator=g) * 0.4 + 0.02], -1).to(DEV)
    dn_mask = _block_mask(N, N)
    if deferred:
        attn_mask = rel.deferred(boxes, boxes, dn_mask)
    else:
        attn_mask = rel(boxes, boxes).flatten(0, 1)
        attn_mask.masked_fill_(dn_mask, float("-inf"))
    qp = x + pos
    out = mod(qp, qp, x, attn_mask=attn_mask)[0]
    w = torch.randn(out.shape, generator=g).to(DEV)
    (out.float() * w).sum().backward()
    grads = {"x": x.grad, "in_proj_weight": mod.in_proj_weight.grad, "in_proj_bias": mod.in_proj_bias.grad,
             "out_proj.weight": mod.out_proj.weight.grad, "out_proj.bias": mod.out_proj.bias.grad,
             "pos_proj.0.weight": rel.pos_proj[0].weight.grad, "pos_proj.0.bias": rel.pos_proj[0].bias.grad}
    return out.detach().float(), grads


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("N", [300, 1100])
def test_module_route_matches_switch_off(rd, monkeypatch, N, deferred):
    from relation_detr_amd import ops
    calls = []
    real = ops.RelationAttentionFunction.apply
    monkeypatch.setattr(ops.RelationAttentionFunction, "apply", lambda *a: calls.append(1) or real(*a))
    out_off, g_off = _module_case(N, deferred, on=False)
    assert not calls
    out_on, g_on = _module_case(N, deferred, on=True)
    assert len(calls) == 1                                            # the new Function ran
    diff = (out_on - out_off).abs()
    assert diff.max().item() < 3e-2 and diff.mean().item() < 3e-3
    for name in g_off:
        assert g_on[name] is not None and g_off[name] is not None, name
        assert _nrel(g_on[name], g_off[name]) <= 2e-2, (name, _nrel(g_on[name], g_off[name]))


def _run_g8_bf16(golden, on):
    from relation_detr_amd import options
    from relation_detr_amd.transformer import build_relation_transformer
    T = torch.from_numpy
    g = golden("g8_transformer_train.npz")
    with options.override(attn_train_fused=on):
        net = build_relation_transformer(num_classes=11, d_ffn=64, enc_layers=2, dec_layers=3, num_queries=24,
                                         hybrid_num_proposals=30)
    net.load_state_dict(synthetic_state_dict(net.state_dict()))
    net = net.to(DEV).to(torch.bfloat16).train()
    bf = lambda t: T(t).to(DEV).to(torch.bfloat16)
    feats = [bf(g[f"feat{i}"]).requires_grad_(True) for i in range(4)]
    masks = [T(g[f"mask{i}"]).to(DEV) for i in range(4)]
    pos = [bf(g[f"pos{i}"]) for i in range(4)]
    dn_label = bf(g["dn_label"]).requires_grad_(True)
    dn_box = T(g["dn_box"]).to(DEV).requires_grad_(True)
    outs = net(feats, masks, pos, dn_label, dn_box, T(g["attn_mask"]).to(DEV))
    loss = sum((o.float() * functional_weights(o.shape, i).to(DEV)).sum() for i, o in enumerate(outs))
    loss.backward()
    grads = {n: p.grad for n, p in net.named_parameters()}
    return [o.detach().float() for o in outs], grads, net


def test_transformer_g8_bf16_training_switch_on_matches_off(rd, golden, monkeypatch):
    """The g8 training configuration in bf16, switch on against switch off.  Outputs agree within 2e-2 normwise.  The
    parameter gradients of this small synthetic configuration in bf16 are themselves far from the fp32 reference (up to ~100 %
    normwise for the switch-off route: bf16 rounding amplified through box refinement and the encoder), so a 2e-2 on/off bound
    on them would measure that amplification, not the attention route.  They are held instead to: the switch-on route is no
    further from the fp32 reference (tests/golden/g8_transformer_train.npz) than 1.25x the switch-off route + 2e-2, for every
    fully recorded gradient and on the mean over all gradient norms."""
    from relation_detr_amd import ops
    from relation_detr_amd.self_attn import RelationSelfAttention
    from helpers import G8_FULL_GRADS
    calls = []
    real = ops.RelationAttentionFunction.apply
    monkeypatch.setattr(ops.RelationAttentionFunction, "apply", lambda *a: calls.append(1) or real(*a))
    outs_off, g_off, _ = _run_g8_bf16(golden, on=False)
    assert not calls
    outs_on, g_on, net = _run_g8_bf16(golden, on=True)
    n_layers = sum(isinstance(m, RelationSelfAttention) for m in net.decoder.modules())
    assert n_layers == 3 and len(calls) == 2 * n_layers              # every decoder layer of the main and the hybrid pass
    for i, (a, b) in enumerate(zip(outs_on, outs_off)):
        assert _nrel(a, b) <= 2e-2, (i, _nrel(a, b))
    g = golden("g8_transformer_train.npz")
    e_on, e_off = [], []
    for n, want in zip((str(x) for x in g["grad_names"]), g["grad_norms"]):
        if g_off[n] is None:
            assert g_on[n] is None, n
            continue
        assert g_on[n] is not None and bool(torch.isfinite(g_on[n]).all()), n
        e_on.append(abs(g_on[n].double().norm().item() - want) / max(1.0, want))
        e_off.append(abs(g_off[n].double().norm().item() - want) / max(1.0, want))
    # per parameter the two bf16 routes scatter around the reference in both directions: held on the mean over all parameters
    assert sum(e_on) / len(e_on) <= 1.25 * sum(e_off) / len(e_off) + 2e-2, (sum(e_on) / len(e_on), sum(e_off) / len(e_off))
    for n in G8_FULL_GRADS:
        ref = torch.from_numpy(g[f"grad.{n}"]).to(DEV)
        e_on, e_off = _nrel(g_on[n], ref), _nrel(g_off[n], ref)
        assert e_on <= 1.25 * e_off + 2e-2, (n, e_on, e_off)
