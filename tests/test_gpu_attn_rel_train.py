"""GPU tests of the bf16 training route that generates the relation bias inside the attention kernels: the forward with the row
log-sum-exp (csrc/attn_rel.hip, relation_attention_boxes_kernel<true>), its backward (csrc/attn_rel_bwd.hip),
``attn_rel_train.relation_attention_boxes_train`` / ``relation_attention_boxes_backward`` / ``RelationAttentionBoxesFunction`` and
``RelationSelfAttention`` / the decoder under ``rel_train_fused``.

Oracle: float64 torch autograd of softmax(Q K^T * scale + relu(conv1x1(sine(box_rel_encoding(src, tgt)))) [, mask]) V built from
oracle/torch_ref.py's restatements, on the same bf16-valued q / k / v / dO, fp32 boxes and fp32 parameters.

The ReLU kink.  The kernels round the sine features to bf16 and use the hardware transcendentals (bias error up to ~2.7e-3 in
a CPU simulation), so the 0.03-0.05 % of pairs whose bias lies within that error of zero switch their ReLU derivative
relative to a float64 oracle; with a random-signed dO that alone is 2-4 % of grad_weight.  That is differentiating at a kink,
not a kernel error, so the backward test removes the ambiguous pairs from BOTH sides with the bool mask:
mask[i, j] = any_{b,h} |pre-activation bias64| < TAU, TAU = 8e-3 (three times the simulated maximum error), asserting first that
this removes at most 25 % of the pairs and no complete row.  The all-active test (proj_bias = 9 > sum |w|) has no kink at all.

Bounds: dq, dk, dv, grad_weight, grad_bias each |err| <= 2^-7 |ref| + 2e-2 max|ref| per element; dq, dk, dv normwise within
1.25 x the old route's error + 1e-3 (old route = _RelationBiasFunction + RelationAttentionFunction on the same inputs);
grad_weight / grad_bias normwise <= 1e-2 against float64 (five times the 2e-3 the simulation gives for the bf16 features alone).
"""
import math

import pytest
import torch

from helpers import G8_FULL_GRADS
from test_gpu_attn_train import C, DEV, H, _block_mask, _check_grad, _inputs, _nrel, _run_g8_bf16

pytestmark = pytest.mark.gpu

TAU = 8e-3


@pytest.fixture(scope="module")
def rd():
    import relation_detr_amd
    from relation_detr_amd import _lib
    _lib.load()


def _boxes(B, N, g):
    return torch.cat([torch.rand(B, N, 2, generator=g), torch.rand(B, N, 2, generator=g) * 0.4 + 0.02], -1).to(DEV)


def _case(B, N, M, seed=0, proj_bias=None):
    """q, k, v, dout as tests/test_gpu_attn_train.py::_inputs; boxes as its _module_case; default Conv2d(64, 8, 1) initialisation."""
    q, k, v, _, _, dout = _inputs(B, N, M, "plain", seed)
    g = torch.Generator().manual_seed(seed + 77 * N + M)
    src, tgt = _boxes(B, N, g), _boxes(B, M, g)
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(64, H, 1)
    w, b = conv.weight.detach().to(DEV), conv.bias.detach().to(DEV)
    if proj_bias is not None:
        b = torch.full_like(b, proj_bias)
    return q, k, v, dout, src, tgt, w, b


def _pre_activation64(src, tgt, w, b):
    from oracle import torch_ref
    feat = torch_ref.sine_embed(torch_ref.box_rel_encoding(src.double(), tgt.double()))            # [B, N, M, 64]
    return torch.einsum("bnmc,hc->bhnm", feat, w.double().reshape(H, -1)) + b.double().view(1, H, 1, 1)


def _oracle(q, k, v, dout, src, tgt, w, b, mask):
    """float64 autograd -> out, lse (natural), dq, dk, dv, grad_weight [H, 64], grad_bias [H]"""
    B, N, _ = q.shape
    M, d = k.shape[1], C // H
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    wd, bd = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    from oracle import torch_ref
    bias = torch_ref.relation_bias(src.double(), tgt.double(), wd, bd)                             # [B, H, N, M]
    x = qd.view(B, N, H, d).transpose(1, 2) @ kd.view(B, M, H, d).transpose(1, 2).transpose(-1, -2) * d ** -0.5 + bias
    if mask is not None:
        x = x.masked_fill(mask, float("-inf"))
    o = (torch.softmax(x, -1) @ vd.view(B, M, H, d).transpose(1, 2)).transpose(1, 2).reshape(B, N, C)
    o.backward(dout.double())
    lse = torch.logsumexp(x.detach(), -1).reshape(B * H, N)
    return o.detach(), lse, qd.grad, kd.grad, vd.grad, wd.grad.reshape(H, -1), bd.grad


def _old_route(q, k, v, dout, src, tgt, w, b, mask):
    """The parent's fastest training route: materialised bias (_RelationBiasFunction) + RelationAttentionFunction."""
    from relation_detr_amd import ops
    from relation_detr_amd.relation import _RelationBiasFunction
    qo, ko, vo = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    wo, bo = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    bias = _RelationBiasFunction.apply(src, tgt, wo, bo, 16, 10000.0, 100.0).flatten(0, 1)
    if mask is not None:
        bias.masked_fill_(mask, float("-inf"))
    out = ops.RelationAttentionFunction.apply(qo, ko, vo, bias, None, H, 1.0 / math.sqrt(C // H))
    out.backward(dout)
    return qo.grad, ko.grad, vo.grad, wo.grad.reshape(H, -1), bo.grad


def _new_route(q, k, v, dout, src, tgt, w, b, mask, packed_qk=False):
    from relation_detr_amd import attn_rel_train as art
    out, lse = art.relation_attention_boxes_train(q, k, v, H, src, tgt, w, b, mask)
    return art.relation_attention_boxes_backward(q, k, v, out, lse, dout, H, src, tgt, w, b, mask, packed_qk=packed_qk)


def _kink_mask(src, tgt, w, b):
    pre = _pre_activation64(src, tgt, w, b)
    kink = (pre.abs() < TAU).any(dim=0).any(dim=0)                                                 # [N, M]
    share = kink.float().mean().item()
    print(f"kink mask: tau {TAU} removes {100 * share:.2f} % of the pairs")
    assert share <= 0.25, share
    assert not kink.all(dim=1).any()
    return kink


def _check_all(case, mask, keep=None, old=True, bias_cancels=False):
    got = _new_route(*case, mask)
    ref = _oracle(*case, mask)[2:]
    was = _old_route(*case, mask) if old else (None,) * 5
    B, N, M = case[0].shape[0], case[0].shape[1], case[1].shape[1]
    for name, gn, go, gr in zip(("dq", "dk", "dv", "grad_weight", "grad_bias"), got, was, ref):
        if keep is not None:
            gn, gr = keep(name, gn), keep(name, gr)
            go = None if go is None else keep(name, go)
        e_new = _nrel(gn, gr)
        e_old = float("nan") if go is None else _nrel(go, gr)
        print(f"B {B} N {N} M {M} mask {mask is not None} {name}: normwise error vs float64 new {e_new:.3e} old {e_old:.3e}")
        err = (gn.double() - gr).abs()
        bound = 2.0 ** -7 * gr.abs() + 2e-2 * gr.abs().max() + 1e-30
        if name in ("dq", "dk", "dv"):
            if go is not None:
                _check_grad(name, gn, go, gr)
            else:
                assert not (err > bound).any(), (name, err.max().item())
        elif name == "grad_bias" and bias_cancels:
            # every unmasked pair active: each row of dS sums to zero, so the reference is 0 up to float64 rounding and gives no
            # scale.  What is left on either route is the rounding of its own P / Di (bf16 out, bf16-rounded row sums), a
            # zero-mean error over 8 heads: the old route's own error is the yardstick, with a factor 2 for the spread of a
            # maximum over 8 samples.
            floor = 2.0 * (go.double() - gr).abs().max()
            print(f"    grad_bias: max |err| new {err.max().item():.3e} old {(go.double() - gr).abs().max().item():.3e}")
            assert not (err > bound + floor).any(), (name, err.max().item(), floor.item())
        else:
            assert not (err > bound).any(), (name, err.max().item(), int((err > bound).sum()))
            assert e_new <= 1e-2, (name, e_new)
    return got


FWD_SHAPES = [(1, 1, 1), (1, 37, 130), (2, 70, 70), (1, 300, 300), (4, 900, 900), (2, 1100, 1100)]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("B,N,M", FWD_SHAPES)
def test_train_forward_is_the_inference_kernel_and_lse(rd, B, N, M, masked):
    from relation_detr_amd import attn_rel_train as art, ops
    q, k, v, dout, src, tgt, w, b = _case(B, N, M)
    mask = _block_mask(N, M) if masked else None
    out, lse = art.relation_attention_boxes_train(q, k, v, H, src, tgt, w, b, mask)
    want = ops.relation_attention_boxes(q, k, v, H, src, tgt, w, b, mask)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))                              # bit for bit
    assert lse.shape == (B * H, N) and lse.dtype == torch.float32
    with torch.no_grad():
        pre = _pre_activation64(src, tgt, w, b).clamp_min(0)
        d = C // H
        x = q.double().view(B, N, H, d).transpose(1, 2) @ k.double().view(B, M, H, d).transpose(1, 2).transpose(-1, -2) * d ** -0.5 + pre
        if mask is not None:
            x = x.masked_fill(mask, float("-inf"))
        ref = torch.logsumexp(x, -1).reshape(B * H, N)
    err = (lse.double() - ref).abs()
    print(f"B {B} N {N} M {M} masked {masked}: max |lse - ref| {err.max().item():.3e}")
    assert not (err > 2.0 ** -7 * ref.abs() + 4e-3).any(), err.max().item()
    import shadow
    assert not (err > shadow.boxes_lse_bound(w, H, B * H).to(err.device)).any(), err.max().item()   # the form the shadow harness holds it to


@pytest.mark.parametrize("masked", [False, True], ids=["kink", "kink+mask"])
@pytest.mark.parametrize("B,N,M", [(1, 37, 130), (2, 70, 70), (1, 300, 300), (2, 1100, 1100)])
def test_backward_matches_float64_and_old_route(rd, B, N, M, masked):
    case = _case(B, N, M)
    mask = _kink_mask(*case[4:])
    if masked:
        mask = mask | _block_mask(N, M)
    _check_all(case, mask)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("B,N,M", [(1, 1, 1), (2, 300, 300), (4, 900, 900), (2, 1500, 1500)])
def test_backward_all_active(rd, B, N, M, masked):
    """proj_bias = 9 > sum |w| (<= 64 / 8 for the default initialisation): every pair is active, no kink, no kink mask."""
    case = _case(B, N, M, proj_bias=9.0)
    assert case[6].abs().sum(dim=(1, 2, 3)).max().item() < 9.0
    _check_all(case, _block_mask(N, M) if masked else None, bias_cancels=True)


def test_backward_is_deterministic(rd):
    case = _case(2, 1100, 1100, seed=3)
    mask = _block_mask(1100, 1100)
    a, b = _new_route(*case, mask), _new_route(*case, mask)
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                           y.contiguous().view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("B,N", [(2, 70), (2, 300)])
def test_fully_masked_row(rd, B, N):
    from relation_detr_amd import attn_rel_train as art
    case = _case(B, N, N)
    q, k, v, dout, src, tgt, w, b = case
    row = 7
    mask = _kink_mask(src, tgt, w, b)
    mask[row, :] = True                                               # one query sees no key (every image and head)
    out, lse = art.relation_attention_boxes_train(q, k, v, H, src, tgt, w, b, mask)
    assert torch.isnan(out[:, row]).all() and torch.isneginf(lse.view(B, H, N)[:, :, row]).all()

    # float64 autograd turns the dead row's NaN into NaN sums (and the old route's backward likewise), so the yardstick is the
    # float64 oracle of the SAME problem without that query: the row contributes nothing to dk, dv, grad_weight, grad_bias
    live = torch.arange(N, device=DEV) != row
    ref = _oracle(q[:, live], k, v, dout[:, live], src[:, live], tgt, w, b, mask[live])[2:]
    got = _new_route(*case, mask)
    assert (got[0][:, row] == 0).all()
    for name, gn, gr in zip(("dq", "dk", "dv", "grad_weight", "grad_bias"), got, ref):
        assert bool(torch.isfinite(gn).all()), name
        gn = gn.double()[:, live] if name == "dq" else gn.double()
        err = (gn - gr).abs()
        assert not (err > 2.0 ** -7 * gr.abs() + 2e-2 * gr.abs().max() + 1e-30).any(), (name, err.max().item())
        if name.startswith("grad_"):
            assert _nrel(gn, gr) <= 1e-2, (name, _nrel(gn, gr))


def test_packed_dq_dk_buffer(rd):
    case = _case(2, 70, 70)
    mask = _block_mask(70, 70)
    dq, dk, dv, gw, gb = _new_route(*case, mask)
    pq, pk, pv, pw, pb = _new_route(*case, mask, packed_qk=True)
    assert pq.data_ptr() + 2 * C == pk.data_ptr() and pq.stride(1) == 2 * C
    for x, y in ((dq, pq), (dk, pk), (dv, pv), (gw, pw), (gb, pb)):
        assert torch.equal(x, y)


def _module_case(N, rel_on, seed=0):
    """tests/test_gpu_attn_train.py::_module_case with a deferred bias and attn_train_fused on, plus the peak allocation of the
    forward + backward above the inputs."""
    from relation_detr_amd import PositionRelationEmbedding, options
    from relation_detr_amd.self_attn import RelationSelfAttention
    torch.manual_seed(0)
    with options.override(attn_train_fused=True, rel_train_fused=rel_on):
        mod = RelationSelfAttention(C, H).to(DEV).to(torch.bfloat16).train()
        rel = PositionRelationEmbedding(16, H).to(DEV).to(torch.bfloat16)
    g = torch.Generator().manual_seed(seed + N)
    B = 2
    x = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    pos = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(DEV)
    boxes = torch.cat([torch.rand(B, N, 2, generator=g), torch.rand(B, N, 2, generator=g) * 0.4 + 0.02], -1).to(DEV)
    dn_mask = _block_mask(N, N)
    qp = x + pos
    wgen = torch.randn(B, N, C, generator=g).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = mod(qp, qp, x, attn_mask=rel.deferred(boxes, boxes, dn_mask))[0]
    (out.float() * wgen).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    grads = {"x": x.grad, "in_proj_weight": mod.in_proj_weight.grad, "in_proj_bias": mod.in_proj_bias.grad,
             "out_proj.weight": mod.out_proj.weight.grad, "out_proj.bias": mod.out_proj.bias.grad,
             "pos_proj.0.weight": rel.pos_proj[0].weight.grad, "pos_proj.0.bias": rel.pos_proj[0].bias.grad}
    return out.detach().float(), grads, peak


@pytest.mark.parametrize("N", [300, 1100])
def test_module_route(rd, monkeypatch, N):
    from relation_detr_amd import attn_rel_train as art
    calls = []
    real = art.RelationAttentionBoxesFunction.apply
    monkeypatch.setattr(art.RelationAttentionBoxesFunction, "apply", lambda *a: calls.append(1) or real(*a))
    out_off, g_off, peak_off = _module_case(N, False)
    assert not calls
    out_on, g_on, peak_on = _module_case(N, True)
    assert len(calls) == 1                                            # the new Function ran exactly once
    one_bias = 4 * 2 * H * N * N
    print(f"N {N}: peak allocation above the inputs, old route {peak_off} B, new route {peak_on} B, one fp32 bias {one_bias} B")
    # no [B*H, N, N] tensor: the new route saves at least the fp32 bias and dbias at any N; below the size of ONE fp32 bias in
    # absolute terms where that quadratic size exceeds the module's other tensors (projections, their gradients, the fp32 loss
    # product: linear in N, ~40 KB per query of the two images), i.e. at the decoder's N = 1100 and not at N = 300
    assert peak_off - peak_on >= 2 * one_bias, (peak_off, peak_on, one_bias)
    if N >= 1100:
        assert peak_on < one_bias, (peak_on, one_bias)
    diff = (out_on - out_off).abs()
    assert diff.max().item() < 3e-2 and diff.mean().item() < 3e-3
    for name in g_off:
        assert g_on[name] is not None and g_off[name] is not None, name
        e = _nrel(g_on[name], g_off[name])
        print(f"N {N} {name}: new route vs old route normwise {e:.3e}")
        assert e <= (1e-1 if name.startswith("pos_proj") else 2e-2), (name, e)


def test_module_takes_the_old_route_when_a_condition_fails(rd, monkeypatch):
    """fp32 modules with the switch on: the deferred bias is materialised exactly as before."""
    from relation_detr_amd import PositionRelationEmbedding, attn_rel_train as art, options
    from relation_detr_amd.self_attn import RelationSelfAttention
    calls = []
    real = art.RelationAttentionBoxesFunction.apply
    monkeypatch.setattr(art.RelationAttentionBoxesFunction, "apply", lambda *a: calls.append(1) or real(*a))
    torch.manual_seed(0)
    with options.override(attn_train_fused=True, rel_train_fused=True):
        mod = RelationSelfAttention(C, H).to(DEV).train()
        rel = PositionRelationEmbedding(16, H).to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 40, C, generator=g).to(DEV).requires_grad_(True)
    boxes = _boxes(2, 40, g)
    out = mod(x, x, x, attn_mask=rel.deferred(boxes, boxes, _block_mask(40, 40)))[0]
    out.sum().backward()
    assert not calls and rel.pos_proj[0].weight.grad is not None and bool(torch.isfinite(x.grad).all())


def _run_g8(golden, rel_on):
    from relation_detr_amd import options
    with options.override(rel_train_fused=rel_on):
        return _run_g8_bf16(golden, on=True)


def test_transformer_g8_bf16_training_switch_on_matches_off(rd, golden, monkeypatch):
    """The g8 training configuration in bf16 with attn_train_fused + rel_train_fused against attn_train_fused alone, by the
    criterion of tests/test_gpu_attn_train.py::test_transformer_g8_bf16_training_switch_on_matches_off."""
    from relation_detr_amd import attn_rel_train as art, ops
    from relation_detr_amd.self_attn import RelationSelfAttention
    new_calls, old_calls = [], []
    real_new, real_old = art.RelationAttentionBoxesFunction.apply, ops.RelationAttentionFunction.apply
    monkeypatch.setattr(art.RelationAttentionBoxesFunction, "apply", lambda *a: new_calls.append(1) or real_new(*a))
    monkeypatch.setattr(ops.RelationAttentionFunction, "apply", lambda *a: old_calls.append(1) or real_old(*a))
    outs_off, g_off, _ = _run_g8(golden, False)
    assert not new_calls
    old_calls.clear()
    outs_on, g_on, net = _run_g8(golden, True)
    n_layers = sum(isinstance(m, RelationSelfAttention) for m in net.decoder.modules())
    assert n_layers == 3
    assert len(new_calls) == n_layers - 1                             # every relation layer of the main pass
    assert len(old_calls) == n_layers + 1                             # its first layer and the hybrid pass
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
    assert sum(e_on) / len(e_on) <= 1.25 * sum(e_off) / len(e_off) + 2e-2, (sum(e_on) / len(e_on), sum(e_off) / len(e_off))
    for n in G8_FULL_GRADS:
        ref = torch.from_numpy(g[f"grad.{n}"]).to(DEV)
        e_on, e_off = _nrel(g_on[n], ref), _nrel(g_off[n], ref)
        assert e_on <= 1.25 * e_off + 2e-2, (n, e_on, e_off)
