"""GPU tests of the fused-producer MSDA backward (csrc/msda_bwd.hip, msda_bwd_fused_kernel) and its training route:
``ops.ms_deform_attn_backward_fused``, ``ops.MultiScaleDeformableAttnFusedFunction`` and ``MultiScaleDeformableAttention`` under
``msda_train_fused``.

Oracle: float64 torch autograd on the CPU through oracle.torch_ref (sampling_locations_from_reference -> softmax -> msda_core),
with the reference points requiring grad.  Bounds:
  fp32  grad_value / grad_logits / grad_ref  atol 1e-4 * max(1, |ref|max); grad_offsets rtol 1e-4 + atol 5e-4 away from
        interpolation kinks (helpers.kink_mask of the oracle's locations)
  bf16  |err| <= 2^-8 * |ref| + 1e-3 * max(1, |ref|max) against the oracle on the bf16-rounded inputs
"""
import numpy as np
import pytest
import torch

from helpers import G8_FULL_GRADS, functional_weights, kink_mask, pyramid, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = torch.from_numpy
SHAPES4 = [(12, 18), (6, 9), (3, 5), (2, 3)]
SHAPES5 = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
SHAPES8 = [(6, 7), (5, 5), (4, 5), (3, 4), (3, 3), (2, 3), (2, 2), (1, 2)]    # S = 120; L*P = 32: every lane stages a point, no padding
SHAPES1 = [(5, 6)]                                                            # S = 30; 28 padding lanes in the softmax
NAN_AT = (0, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def rd():
    import relation_detr_amd
    from relation_detr_amd import _lib
    _lib.load()
    return relation_detr_amd


def producer_inputs(B, Nq, shapes, ref_dim, seed, dtype=torch.float32, nan=True):
    """value, raw offsets / logits (value's dtype), reference points (fp32), grad_out; some points outside their level, one NaN
    offset (the oracle gets a far-outside offset there)."""
    g = torch.Generator().manual_seed(seed)
    shp, start, S = pyramid(shapes)
    L = shp.shape[0]
    value = torch.randn(B, S, 8, 32, generator=g)
    offsets = torch.randn(B, Nq, 8, L, 4, 2, generator=g) * (1.0 if ref_dim == 2 else 2.0)
    logits = torch.randn(B, Nq, 8, L * 4, generator=g) * 2.0
    if ref_dim == 2:
        ref = torch.rand(B, Nq, L, 2, generator=g) * 1.2 - 0.1
    else:
        ref = torch.cat([torch.rand(B, Nq, L, 2, generator=g) * 1.1 - 0.05, torch.rand(B, Nq, L, 2, generator=g) * 0.45 + 0.05], -1)
    go = torch.randn(B, Nq, 256, generator=g)
    value, offsets, logits, go = (t.to(dtype) for t in (value, offsets, logits, go))
    off_oracle = offsets.double()
    if nan:
        offsets[NAN_AT] = float("nan")
        off_oracle[NAN_AT] = -1000.0
    return value, shp, start, offsets, logits, ref, go, off_oracle


def oracle(value, shp, offsets, logits, ref, go):
    """float64 autograd -> out, grad_value, grad_offsets, grad_logits, grad_ref, locations"""
    from oracle import torch_ref
    v, o, lg, r = (t.detach().double().clone().requires_grad_(True) for t in (value, offsets, logits, ref))
    B, Nq, H, L, P, _ = o.shape
    loc = torch_ref.sampling_locations_from_reference(r, o, shp, P)
    w = lg.softmax(-1).view(B, Nq, H, L, P)
    out = torch_ref.msda_core(v, shp, loc, w)
    out.backward(go.double())
    return out.detach(), v.grad, o.grad, lg.grad, r.grad, loc.detach()


def _n(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def close_abs(got, want, what):
    got, want = _n(got), _n(want)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4 * max(1.0, float(np.abs(want).max())), err_msg=what)


def close_bf16(got, want, what, mask=None):
    got, want = _n(got), _n(want)
    err = np.abs(got - want)
    bound = 2.0 ** -8 * np.abs(want) + 1e-3 * max(1.0, float(np.abs(want).max()))
    ok = err <= bound
    if mask is not None:
        ok |= ~mask
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} outside, worst excess {float((err - bound).max()):.3e}"


def close_offsets(got, want, loc, shp, what):
    mask = kink_mask(_n(loc), shp.numpy())
    got, want = _n(got)[mask], _n(want)[mask]
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=5e-4, err_msg=what)


def ref_mask(loc, shp):
    """(b, q, l) entries of grad_ref away from every kink of their 8 x 4 points (grad_ref sums their location gradients)"""
    return kink_mask(_n(loc), shp.numpy()).all(axis=(2, 4, 5))[..., None]


def kept_enough(shapes, loc, shp):
    """The two added level counts: the kink masks keep at least 99 % of the offset elements and 75 % of the reference-point
    entries, so that a mask cannot hide a failure."""
    if shapes in (SHAPES8, SHAPES1):
        kinks, refs = kink_mask(_n(loc), shp.numpy()).mean(), ref_mask(loc, shp).mean()
        print(f"L = {len(shapes)}: offsets kept {kinks:.4f}, reference entries kept {refs:.4f}")
        assert kinks >= 0.99 and refs >= 0.75, (kinks, refs)


def run_fused(value, shp, start, offsets, logits, ref, go, deterministic=False):
    from relation_detr_amd import ops
    args = [t.to(DEV).contiguous() for t in (value, shp, start, offsets, logits, ref, go)]
    res = ops.ms_deform_attn_backward_fused(*args, deterministic=deterministic, need_ref_grad=True)
    torch.cuda.synchronize()
    return res


# Nq = 11: one full block of 8 queries and a tail whose last wave holds a single valid query
CASES = [(SHAPES4, 2, 37, 2), (SHAPES4, 1, 70, 4), (SHAPES5, 2, 37, 4), (SHAPES5, 1, 70, 2), ([(9, 13), (5, 7), (3, 4)], 2, 24, 2),
         (SHAPES8, 2, 11, 2), (SHAPES8, 2, 11, 4), (SHAPES1, 2, 11, 2), (SHAPES1, 2, 11, 4)]


@pytest.mark.parametrize("shapes,B,Nq,ref_dim", CASES)
@pytest.mark.parametrize("deterministic", [False, True])
def test_fused_backward_fp32_matches_oracle(rd, shapes, B, Nq, ref_dim, deterministic):
    value, shp, start, off, lg, ref, go, off_o = producer_inputs(B, Nq, shapes, ref_dim, seed=Nq + ref_dim)
    gv, goff, glg, gref = run_fused(value, shp, start, off, lg, ref, go, deterministic)
    assert gv.dtype == torch.float32 and goff.dtype == torch.float32 and glg.dtype == torch.float32
    assert tuple(gref.shape) == (B, Nq, len(shapes), ref_dim)
    _, rv, ro, rl, rr, loc = oracle(value, shp, off_o, lg, ref, go)
    kept_enough(shapes, loc, shp)
    close_abs(gv, rv, "grad_value")
    close_abs(glg, rl, "grad_logits")
    assert goff[NAN_AT].item() == 0.0                       # the NaN point contributes nothing
    close_offsets(goff, ro, loc, shp, "grad_offsets")
    m = ref_mask(loc, shp)
    np.testing.assert_allclose(_n(gref) * m, _n(rr) * m, rtol=0, atol=1e-4 * max(1.0, float(np.abs(_n(rr)).max())),
                               err_msg="grad_reference_points")


@pytest.mark.parametrize("shapes,B,Nq,ref_dim", CASES)
def test_fused_backward_bf16_matches_oracle(rd, shapes, B, Nq, ref_dim):
    value, shp, start, off, lg, ref, go, off_o = producer_inputs(B, Nq, shapes, ref_dim, seed=Nq + ref_dim + 100,
                                                                 dtype=torch.bfloat16)
    gv, goff, glg, gref = run_fused(value, shp, start, off, lg, ref, go)
    assert gv.dtype == torch.float32 and goff.dtype == torch.bfloat16 and glg.dtype == torch.bfloat16
    _, rv, ro, rl, rr, loc = oracle(value.double(), shp, off_o, lg.double(), ref, go.double())
    kinks = kink_mask(_n(loc), shp.numpy())
    kept_enough(shapes, loc, shp)
    close_bf16(gv, rv, "grad_value")
    close_bf16(glg, rl, "grad_logits")
    close_bf16(goff, ro, "grad_offsets", kinks)
    close_bf16(gref, rr, "grad_reference_points", np.broadcast_to(ref_mask(loc, shp), rr.shape))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shapes,ref_dim", [(SHAPES4, 2), (SHAPES5, 4), ([(9, 13), (5, 7), (3, 4)], 2)])
def test_fused_function_forward_is_the_eval_kernel(rd, dtype, shapes, ref_dim):
    from relation_detr_amd import ops
    value, shp, start, off, lg, ref, _, _ = producer_inputs(2, 45, shapes, ref_dim, seed=7, dtype=dtype)
    args = [t.to(DEV).contiguous() for t in (value, shp, start, off, lg, ref)]
    want = ops.ms_deform_attn_forward_fused(*args, algo="direct")
    leaves = [a.clone().requires_grad_(True) if i in (0, 3, 4, 5) else a for i, a in enumerate(args)]
    got = ops.MultiScaleDeformableAttnFusedFunction.apply(*leaves)
    assert got.dtype == dtype and torch.equal(got.detach(), want)
    got.float().sum().backward()
    assert all(leaves[i].grad is not None and leaves[i].grad.dtype == leaves[i].dtype for i in (0, 3, 4, 5))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fused_backward_deterministic_mode(rd, dtype, ref_dim):
    from relation_detr_amd import ops
    value, shp, start, off, lg, ref, go, _ = producer_inputs(2, 70, SHAPES4, ref_dim, seed=11, dtype=dtype)
    d1 = run_fused(value, shp, start, off, lg, ref, go, deterministic=True)
    d2 = run_fused(value, shp, start, off, lg, ref, go, deterministic=True)
    a = run_fused(value, shp, start, off, lg, ref, go, deterministic=False)
    assert all(torch.equal(x, y) for x, y in zip(d1, d2))
    assert torch.equal(d1[1], a[1]) and torch.equal(d1[2], a[2]) and torch.equal(d1[3], a[3])
    np.testing.assert_allclose(d1[0].cpu().numpy(), a[0].cpu().numpy(), rtol=1e-5, atol=1e-4)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        args = [t.to(DEV).contiguous() for t in (value, shp, start, off, lg, ref)]
        v = args[0].clone().requires_grad_(True)
        out = ops.MultiScaleDeformableAttnFusedFunction.apply(v, *args[1:])
        out.backward(go.to(DEV))
        assert torch.equal(v.grad, d1[0].to(dtype))
    finally:
        torch.use_deterministic_algorithms(was)


def materialised_route(value, shp, start, off, lg, ref, go):
    """The existing GPU training route on fp32 copies of the inputs: torch producer + MultiScaleDeformableAttnFunction + autograd."""
    from relation_detr_amd import ops
    from relation_detr_amd.ms_deform_attn import sampling_locations
    v, o, l_, r = (t.to(DEV).float().contiguous().requires_grad_(True) for t in (value, off, lg, ref))
    B, Nq, H, L, P, _ = o.shape
    loc = sampling_locations(r, o, shp.to(DEV), P)
    w = l_.softmax(-1).view(B, Nq, H, L, P)
    out = ops.MultiScaleDeformableAttnFunction.apply(v, shp.to(DEV), start.to(DEV), loc.contiguous(), w.contiguous(), 64)
    out.backward(go.to(DEV).float())
    return v.grad, o.grad, l_.grad, r.grad, loc.detach()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_backward_encoder_shape_matches_materialised_route(rd, dtype):
    import bench
    shapes = [tuple(s) for s in bench.R50_SHAPES]
    _, _, S = pyramid(shapes)
    value, shp, start, off, lg, ref, go, _ = producer_inputs(1, S, shapes, 2, seed=5, dtype=dtype, nan=False)
    gv, goff, glg, gref = run_fused(value, shp, start, off, lg, ref, go)
    rv, ro, rl, rr, loc = materialised_route(value, shp, start, off, lg, ref, go)
    kinks = kink_mask(_n(loc), shp.numpy())
    if dtype == torch.float32:
        close_abs(gv, rv, "grad_value")
        close_abs(glg, rl, "grad_logits")
        close_offsets(goff, ro, loc, shp, "grad_offsets")
        m = ref_mask(loc, shp)
        np.testing.assert_allclose(_n(gref) * m, _n(rr) * m, rtol=0, atol=1e-4 * max(1.0, float(np.abs(_n(rr)).max())))
    else:
        close_bf16(gv, rv, "grad_value")
        close_bf16(glg, rl, "grad_logits")
        close_bf16(goff, ro, "grad_offsets", kinks)
        close_bf16(gref, rr, "grad_reference_points", np.broadcast_to(ref_mask(loc, shp), gref.shape))


def test_fused_backward_decoder_shape_matches_materialised_route(rd):
    import bench
    shapes = [tuple(s) for s in bench.R50_SHAPES]
    value, shp, start, off, lg, ref, go, _ = producer_inputs(2, 900, shapes, 4, seed=6, nan=False)
    gv, goff, glg, gref = run_fused(value, shp, start, off, lg, ref, go)
    rv, ro, rl, rr, loc = materialised_route(value, shp, start, off, lg, ref, go)
    close_abs(gv, rv, "grad_value")
    close_abs(glg, rl, "grad_logits")
    close_offsets(goff, ro, loc, shp, "grad_offsets")
    m = ref_mask(loc, shp)
    np.testing.assert_allclose(_n(gref) * m, _n(rr) * m, rtol=0, atol=1e-4 * max(1.0, float(np.abs(_n(rr)).max())))


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_module_training_route_matches_materialised_route(rd, ref_dim):
    from relation_detr_amd import MultiScaleDeformableAttention, options
    torch.manual_seed(0)
    shp, start, S = pyramid(SHAPES4)
    B, Nq = 2, 45
    with options.override(msda_train_fused=False):
        base = MultiScaleDeformableAttention(256, 4, 8, 4).to(DEV).train()
    with options.override(msda_train_fused=True):
        fused = MultiScaleDeformableAttention(256, 4, 8, 4).to(DEV).train()
    with torch.no_grad():                      # non-trivial offsets / logits projections
        for p in base.parameters():
            p.add_(torch.randn_like(p) * 0.02)
    fused.load_state_dict(base.state_dict())
    g = torch.Generator().manual_seed(3)
    query = torch.randn(B, Nq, 256, generator=g)
    value = torch.randn(B, S, 256, generator=g)
    if ref_dim == 2:
        ref = torch.rand(B, Nq, 4, 2, generator=g)
    else:
        ref = torch.cat([torch.rand(B, Nq, 4, 2, generator=g), torch.rand(B, Nq, 4, 2, generator=g) * 0.4 + 0.05], -1)
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[1, -20:] = True
    go = torch.randn(B, Nq, 256, generator=g).to(DEV)
    res = []
    for mod in (base, fused):
        q, v, r = (t.to(DEV).clone().requires_grad_(True) for t in (query, value, ref))
        out = mod(q, r, v, shp.to(DEV), start.to(DEV), mask.to(DEV))
        out.backward(go)
        res.append((out.detach(), q.grad, v.grad, r.grad, {n: p.grad for n, p in mod.named_parameters()}))
    (o0, q0, v0, r0, p0), (o1, q1, v1, r1, p1) = res
    close_abs(o1, o0, "output")
    close_abs(q1, q0, "d / d query")
    close_abs(v1, v0, "d / d value")
    close_abs(r1, r0, "d / d reference_points")
    for n in p0:
        close_abs(p1[n], p0[n], n)


def test_module_takes_the_fused_route_only_when_switched_on(rd, monkeypatch):
    from relation_detr_amd import MultiScaleDeformableAttention, ops, options
    calls = []
    real = ops.MultiScaleDeformableAttnFusedFunction.apply
    monkeypatch.setattr(ops.MultiScaleDeformableAttnFusedFunction, "apply", lambda *a: calls.append(1) or real(*a))
    shp, start, S = pyramid(SHAPES4)
    x = torch.randn(1, S, 256, device=DEV)
    ref = torch.rand(1, S, 4, 2, device=DEV)
    for on in (False, True):
        with options.override(msda_train_fused=on):
            mod = MultiScaleDeformableAttention().to(DEV).train()
        mod(x, ref, x, shp.to(DEV), start.to(DEV), None).sum().backward()
        assert len(calls) == int(on)
    with torch.no_grad():                       # inference keeps the fused forward without autograd
        mod(x, ref, x, shp.to(DEV), start.to(DEV), None)
    assert len(calls) == 1


def _run_transformer(golden, device):
    from relation_detr_amd import options
    from relation_detr_amd.transformer import build_relation_transformer
    g = golden("g8_transformer_train.npz")
    with options.override(msda_train_fused=True):
        net = build_relation_transformer(num_classes=11, d_ffn=64, enc_layers=2, dec_layers=3, num_queries=24,
                                         hybrid_num_proposals=30)
    assert all(m.options.msda_train_fused for m in net.modules() if hasattr(m, "options"))
    net.load_state_dict(synthetic_state_dict(net.state_dict()))
    net = net.to(device).train()
    feats = [T(g[f"feat{i}"]).to(device).requires_grad_(True) for i in range(4)]
    masks = [T(g[f"mask{i}"]).to(device) for i in range(4)]
    pos = [T(g[f"pos{i}"]).to(device) for i in range(4)]
    dn_label = T(g["dn_label"]).to(device).requires_grad_(True)
    dn_box = T(g["dn_box"]).to(device).requires_grad_(True)
    outs = net(feats, masks, pos, dn_label, dn_box, T(g["attn_mask"]).to(device))
    assert len(outs) == 8 and all(o is not None for o in outs)
    loss = sum((o.float() * functional_weights(o.shape, i).to(device)).sum() for i, o in enumerate(outs))
    loss.backward()
    return g, net, outs, loss, feats, dn_label, dn_box


def _check_transformer(g, net, outs, loss, feats, dn_label, dn_box, atol, gtol):
    for i, o in enumerate(outs):
        assert tuple(o.shape) == g[f"out{i}"].shape
        np.testing.assert_allclose(o.detach().float().cpu().numpy(), g[f"out{i}"], rtol=0, atol=atol, err_msg=f"output {i}")
    assert abs(loss.item() - float(g["loss"])) <= 200 * atol
    params = dict(net.named_parameters())
    names = [str(n) for n in g["grad_names"]]
    assert list(params) == names
    for n, want in zip(names, g["grad_norms"]):
        got = 0.0 if params[n].grad is None else params[n].grad.double().norm().item()
        assert abs(got - want) <= gtol * max(1.0, want), (n, got, want)

    def close(got, want, what):
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(got.detach().float().cpu().numpy(), want, rtol=0, atol=gtol * scale, err_msg=what)
    for n in G8_FULL_GRADS:
        close(params[n].grad, g[f"grad.{n}"], n)
    close(feats[3].grad, g["grad_feat3"], "d loss / d level-3 features")
    assert abs(feats[0].grad.double().norm().item() - float(g["grad_feat0_norm"])) <= gtol * max(1.0, float(g["grad_feat0_norm"]))
    close(dn_label.grad, g["grad_dn_label"], "d loss / d denoising label queries")
    close(dn_box.grad, g["grad_dn_box"], "d loss / d denoising box queries")


def test_transformer_training_on_the_fused_route_matches_reference(rd, golden, monkeypatch):
    from relation_detr_amd import ops
    calls = []
    real = ops.MultiScaleDeformableAttnFusedFunction.apply
    monkeypatch.setattr(ops.MultiScaleDeformableAttnFusedFunction, "apply", lambda *a: calls.append(1) or real(*a))
    res = _run_transformer(golden, DEV)
    assert calls                                   # the MSDA cores of the harness took the fused training route
    _check_transformer(*res, atol=5e-4, gtol=2e-3)
