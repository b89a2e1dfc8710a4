"""GPU tests of the add + LayerNorm training route (relation_detr_amd/ln_train.py, csrc/layernorm.hip): the forward that keeps the
row statistics, the one-pass backward with its fixed-order parameter-gradient reduction, ``AddLayerNormFunction`` and the routing of
``transformer.add_norm`` / the encoder and decoder layers under ``ln_train_fused``.

Reference: float64 autograd of ``F.layer_norm(x + r, (256,), gamma, beta, eps)`` on the STORED (bf16-rounded) input values, never
the code under test.  Errors are norm-wise, ``|got - ref| / |ref|`` over the whole tensor (for the statistics: over the column of
means / of rstds -- a single row's mean of 256 N(0, 2) values may be arbitrarily close to zero, where no relative bound on that one
number can hold).  Bounds:
  bf16 out, dx, dgamma, dbeta   2^-8: a correctly rounded bf16 result is within 2^-9 per element, a factor of two on top; dropping
                                either mean term of dx costs about 1/16
  fp32 out, dx                  1e-5
  fp32 dgamma, dbeta            1e-6 + 4 * 2^-24 * sqrt(rows): the random-walk growth of an fp32 running sum, a factor of four
  stats                         1e-5
"""
import dataclasses
import functools
import os

import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-5


@pytest.fixture(scope="module")
def ln():
    from relation_detr_amd import _lib, ln_train
    _lib.load()
    return ln_train


def _big_rows():
    from relation_detr_amd import ln_train
    return 16 * ln_train.MAX_PARTIALS * 2 + 5            # the grid stride takes more than two trips, with a ragged tail


ROWS = [1, 15, 16, 17, 257, "big"]
VARIANTS = ["plain", "no_residual", "sliced_x", "expanded_dy"]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def nrel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def case(dtype, rows, variant):
    """Inputs in the storage dtype on the device and the float64 reference on their stored values; built once, never modified."""
    rows = _big_rows() if rows == "big" else rows
    g = torch.Generator(device=DEV).manual_seed(1000 + rows)
    randn = lambda *shape: torch.randn(*shape, generator=g, device=DEV)
    wide = randn(rows, 768).to(dtype)
    x = wide[:, 256:512] if variant == "sliced_x" else wide[:, 256:512].contiguous()
    r = None if variant == "no_residual" else randn(rows, 256).to(dtype)
    if variant == "expanded_dy":
        dy = torch.ones((), dtype=dtype, device=DEV).expand(rows, 256)            # what out.sum().backward() hands down
    else:
        dy = randn(rows, 256).to(dtype)
    gamma = (1 + 0.1 * randn(256)).to(dtype)
    beta = (0.1 * randn(256)).to(dtype)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    r64 = None if r is None else r.double().requires_grad_(True)
    s64 = x64 if r64 is None else x64 + r64
    out64 = F.layer_norm(s64, (256,), g64, b64, EPS)
    out64.backward(dy.double())
    with torch.no_grad():
        mean = s64.mean(-1)
        rstd = (s64.var(-1, unbiased=False) + EPS).rsqrt()
    if r64 is not None:
        assert torch.equal(x64.grad, r64.grad)
    ref = dict(out=out64.detach(), dx=x64.grad, dgamma=g64.grad, dbeta=b64.grad, mean=mean, rstd=rstd)
    return dict(rows=rows, x=x, r=r, dy=dy, gamma=gamma, beta=beta, ref=ref)


@functools.lru_cache(maxsize=None)
def new_route(dtype, rows, variant):
    from relation_detr_amd import ln_train
    c = case(dtype, rows, variant)
    out, stats = ln_train.add_layer_norm_train(c["x"], c["r"], c["gamma"], c["beta"], EPS)
    dx, dgamma, dbeta = ln_train.add_layer_norm_backward(c["dy"], c["x"], c["r"], stats, c["gamma"])
    torch.cuda.synchronize()
    return dict(out=out, stats=stats, dx=dx, dgamma=dgamma, dbeta=dbeta)


def torch_route(c):
    """norm(x + r) under autograd on the device, in the storage dtype: what `add_norm` does with the option off."""
    x, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (c["x"], c["gamma"], c["beta"]))
    r = None if c["r"] is None else c["r"].detach().clone().requires_grad_(True)
    out = F.layer_norm(x if r is None else x + r, (256,), gamma, beta, EPS)
    out.backward(c["dy"])
    return dict(out=out.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)


PARAMS = [(d, n, v) for d in (BF, F32) for n in ROWS for v in VARIANTS]
IDS = [f"{'bf16' if d == BF else 'fp32'}-{n}-{v}" for d, n, v in PARAMS]


@pytest.mark.parametrize("dtype,rows,variant", PARAMS, ids=IDS)
def test_forward_has_the_inference_bits_and_the_row_statistics(ln, dtype, rows, variant):
    from relation_detr_amd import ops
    c, got = case(dtype, rows, variant), new_route(dtype, rows, variant)
    with torch.no_grad():
        want = ops.add_layer_norm(c["x"], c["r"], c["gamma"], c["beta"], EPS)
    assert got["out"].shape == c["x"].shape and got["out"].is_contiguous()
    assert same_bits(got["out"], want)
    stats = got["stats"]
    assert stats.dtype == F32 and tuple(stats.shape) == (c["rows"], 2)
    e_mean, e_rstd = nrel(stats[:, 0], c["ref"]["mean"]), nrel(stats[:, 1], c["ref"]["rstd"])
    print(f"\nstats rows {c['rows']}: mean {e_mean:.2e} rstd {e_rstd:.2e} (bound 1e-5)")
    assert e_mean <= 1e-5 and e_rstd <= 1e-5, (e_mean, e_rstd)


@pytest.mark.parametrize("dtype,rows,variant", PARAMS, ids=IDS)
def test_accuracy_against_float64(ln, dtype, rows, variant):
    c, got = case(dtype, rows, variant), new_route(dtype, rows, variant)
    old = torch_route(c)
    n = c["rows"]
    if dtype == BF:
        bound = dict(out=2.0 ** -8, dx=2.0 ** -8, dgamma=2.0 ** -8, dbeta=2.0 ** -8)
    else:
        bound = dict(out=1e-5, dx=1e-5, dgamma=1e-6 + 4 * 2.0 ** -24 * n ** 0.5, dbeta=1e-6 + 4 * 2.0 ** -24 * n ** 0.5)
    err = {}
    for name in ("out", "dx", "dgamma", "dbeta"):
        assert got[name].dtype == dtype and got[name].shape == c["ref"][name].shape
        err[name] = nrel(got[name], c["ref"][name])
        e_old = nrel(old[name], c["ref"][name])
        ratio = err[name] / e_old if e_old > 0 else float("inf") if err[name] > 0 else 1.0
        print(f"\n{name:6s} rows {n:6d}: new {err[name]:.3e} (bound {bound[name]:.3e})  torch route {e_old:.3e}  new / torch {ratio:.2f}", end="")
    print()
    bad = {k: (v, bound[k]) for k, v in err.items() if not v <= bound[k]}
    assert not bad, bad


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_gradient_sharing(ln, dtype):
    c, direct = case(dtype, 257, "plain"), new_route(dtype, 257, "plain")

    def leaves(**grad):
        return {k: c[k].detach().clone().requires_grad_(grad.get(k, True)) for k in ("x", "r", "gamma", "beta")}
    # both operands: the same gradient, the bits of the direct call
    t = leaves()
    out = ln.AddLayerNormFunction.apply(t["x"], t["r"], t["gamma"], t["beta"], EPS)
    assert same_bits(out, direct["out"])
    out.backward(c["dy"])
    assert same_bits(t["x"].grad, t["r"].grad) and same_bits(t["x"].grad, direct["dx"])
    assert same_bits(t["gamma"].grad, direct["dgamma"]) and same_bits(t["beta"].grad, direct["dbeta"])
    # x and residual the same leaf: twice dx
    leaf = c["x"].detach().clone().requires_grad_(True)
    two = ln.AddLayerNormFunction.apply(leaf, leaf, t["gamma"].detach(), t["beta"].detach(), EPS)
    _, stats = ln.add_layer_norm_train(leaf, leaf, c["gamma"], c["beta"], EPS)
    dx_two, _, _ = ln.add_layer_norm_backward(c["dy"], leaf, leaf, stats, c["gamma"], need_params=False)
    two.backward(c["dy"])
    assert same_bits(leaf.grad, dx_two + dx_two)
    # residual without a gradient: only x gets one
    t = leaves(r=False)
    ln.AddLayerNormFunction.apply(t["x"], t["r"], t["gamma"], t["beta"], EPS).backward(c["dy"])
    assert t["r"].grad is None and same_bits(t["x"].grad, direct["dx"])
    # frozen parameters: no parameter gradient, dx unchanged bit for bit
    t = leaves(gamma=False, beta=False)
    ln.AddLayerNormFunction.apply(t["x"], t["r"], t["gamma"], t["beta"], EPS).backward(c["dy"])
    assert t["gamma"].grad is None and t["beta"].grad is None
    assert same_bits(t["x"].grad, direct["dx"]) and same_bits(t["r"].grad, direct["dx"])
    # only the parameters
    t = leaves(x=False, r=False)
    ln.AddLayerNormFunction.apply(t["x"], t["r"], t["gamma"], t["beta"], EPS).backward(c["dy"])
    assert t["x"].grad is None and t["r"].grad is None
    assert same_bits(t["gamma"].grad, direct["dgamma"]) and same_bits(t["beta"].grad, direct["dbeta"])
    # no residual at all
    cn, dn = case(dtype, 257, "no_residual"), new_route(dtype, 257, "no_residual")
    xs = cn["x"].detach().clone().requires_grad_(True)
    ln.AddLayerNormFunction.apply(xs, None, cn["gamma"], cn["beta"], EPS).backward(cn["dy"])
    assert same_bits(xs.grad, dn["dx"])


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_backward_is_deterministic(ln, dtype):
    c, first = case(dtype, "big", "plain"), new_route(dtype, "big", "plain")
    dx, dgamma, dbeta = ln.add_layer_norm_backward(c["dy"], c["x"], c["r"], first["stats"], c["gamma"])
    assert same_bits(dx, first["dx"]) and same_bits(dgamma, first["dgamma"]) and same_bits(dbeta, first["dbeta"])


def test_add_norm_takes_the_route_only_where_it_applies(ln, monkeypatch):
    from relation_detr_amd import options
    from relation_detr_amd.transformer import add_norm
    calls = []
    real = ln.AddLayerNormFunction.apply
    monkeypatch.setattr(ln.AddLayerNormFunction, "apply", lambda *a: calls.append(1) or real(*a))
    on = dataclasses.replace(options.Options(), ln_train_fused=True)
    off = dataclasses.replace(options.Options(), ln_train_fused=False)

    def run(opts, C=256, dtype=BF, grad=True, residual=True, use_out=False):
        torch.manual_seed(0)
        norm = torch.nn.LayerNorm(C).to(DEV).to(dtype)
        x = torch.randn(2, 9, C, device=DEV).to(dtype).requires_grad_(True)
        r = torch.randn(2, 9, C, device=DEV).to(dtype).requires_grad_(True) if residual else None
        out = torch.empty(2, 9, C, device=DEV, dtype=dtype) if use_out else None
        before = len(calls)
        with torch.enable_grad() if grad else torch.no_grad():
            y = add_norm(norm, x, r, out=out, opts=opts)
            if grad:
                y.float().square().sum().backward()
                assert x.grad is not None and norm.weight.grad is not None and norm.bias.grad is not None
                assert all(torch.isfinite(t.grad.float()).all() for t in (x, norm.weight, norm.bias))
                assert r is None or torch.equal(r.grad, x.grad)
        with torch.no_grad():
            want = norm(x if r is None else x + r)
        assert (y.float() - want.float()).abs().max() <= 2.0 ** -6 * max(1.0, float(want.float().abs().max()))
        assert out is None or y is out
        return len(calls) - before

    assert run(off) == 0
    assert run(on) == 1
    assert run(on, dtype=F32) == 1
    assert run(on, residual=False) == 1
    assert run(on, use_out=True) == 1
    assert run(on, grad=False) == 0                        # under no_grad: the inference kernel
    assert run(on, C=128) == 0
    assert run(on, dtype=torch.float16) == 0
    with options.override(ln_train_fused=True):            # without `opts`: the process-level object
        assert run(None) == 1
    assert run(None) == 0
    assert len(calls) == 5


# ------------------------------------------------------------------------------------------------------------ layers
LAYER_SHAPES = [(8, 10), (4, 5), (2, 3), (1, 2)]


def _layer_state(layer, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                      # non-trivial projections, distinct LayerNorm parameters; weights that bf16 holds exactly
        for m in layer.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
        for p in layer.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.02)
            p.copy_(p.to(BF).float())
    return layer.state_dict()


def _run_layer(kind, layer, inputs, dtype):
    from helpers import pyramid
    shp, start, S = pyramid(LAYER_SHAPES)
    shp, start = shp.to(DEV), start.to(DEV)
    cast = lambda t: t.to(DEV).to(dtype).requires_grad_(True)
    if kind == "encoder":
        query, pos, ref, go = inputs
        q, p = cast(query), cast(pos)
        r = ref.to(DEV).requires_grad_(True)
        out = layer(q, p, r, shp, start)
        leaves = {"d/d query": q, "d/d query_pos": p, "d/d reference_points": r}
    else:
        query, pos, ref, value, go = inputs
        q, p, v = cast(query), cast(pos), cast(value)
        r = ref.to(DEV).requires_grad_(True)
        out = layer(q, p, r, v, shp, start)
        leaves = {"d/d query": q, "d/d query_pos": p, "d/d reference_points": r, "d/d value": v}
    out.backward(go.to(DEV).to(dtype))
    res = {"output": out.detach()}
    res.update({k: t.grad for k, t in leaves.items()})
    res.update({n: p.grad for n, p in layer.named_parameters()})
    return res


def _layer_inputs(kind):
    from helpers import pyramid
    _, _, S = pyramid(LAYER_SHAPES)
    g = torch.Generator().manual_seed(7)
    B, N = 2, 24
    if kind == "encoder":
        return (torch.randn(B, S, 256, generator=g).to(BF), torch.randn(B, S, 256, generator=g).to(BF),
                torch.rand(B, S, 4, 2, generator=g), torch.randn(B, S, 256, generator=g).to(BF))
    ref = torch.cat([torch.rand(B, N, 4, 2, generator=g), torch.rand(B, N, 4, 2, generator=g) * 0.4 + 0.05], -1)
    return (torch.randn(B, N, 256, generator=g).to(BF), torch.randn(B, N, 256, generator=g).to(BF), ref,
            torch.randn(B, S, 256, generator=g).to(BF), torch.randn(B, N, 256, generator=g).to(BF))


def _layer_table(kind, monkeypatch):
    from relation_detr_amd import ln_train, options
    from relation_detr_amd.transformer import RelationTransformerDecoderLayer, RelationTransformerEncoderLayer
    cls = RelationTransformerEncoderLayer if kind == "encoder" else RelationTransformerDecoderLayer
    calls = []
    real = ln_train.AddLayerNormFunction.apply
    monkeypatch.setattr(ln_train.AddLayerNormFunction, "apply", lambda *a: calls.append(1) or real(*a))
    torch.manual_seed(0)
    with options.override(ln_train_fused=False):
        base = cls().train()
    state = _layer_state(base, 5)
    base = base.to(DEV)
    layers = {}
    for key, on in (("a", False), ("b", True)):
        with options.override(ln_train_fused=on):
            m = cls()
        m.load_state_dict(state)
        layers[key] = m.to(DEV).to(BF).train()
    inputs = _layer_inputs(kind)
    want = _run_layer(kind, base, inputs, F32)
    assert not calls
    got = {"a": _run_layer(kind, layers["a"], inputs, BF)}
    assert not calls
    got["b"] = _run_layer(kind, layers["b"], inputs, BF)
    assert len(calls) == (2 if kind == "encoder" else 3)               # every norm of the layer
    lines = [f"{kind + ' layer: tensor':44s} {'err_a (torch route)':>22s} {'err_b (ln_train_fused)':>24s}"]
    bad = []
    for name, ref in want.items():
        if ref is None:                                  # a parameter the layer does not use on this call: on no route
            assert got["a"][name] is None and got["b"][name] is None, name
            continue
        assert got["a"][name] is not None and got["b"][name] is not None, name
        scale = max(1.0, float(ref.abs().max()))
        ea, eb = (float((got[k][name].float() - ref.float()).abs().max()) / scale for k in ("a", "b"))
        lines.append(f"{name:44s} {ea:22.3e} {eb:24.3e}")
        if not eb <= 1.5 * ea + 2.0 ** -9:
            bad.append(name)
    return "\n".join(lines), bad


def test_layers_are_as_accurate_as_on_the_torch_route(ln, monkeypatch):
    """fp32 with the option off (the same weights) is the reference; per tensor the worst |err| / max(1, max|ref|) of bf16 training
    with ``ln_train_fused`` (b) against bf16 training without (a): err_b <= 1.5 * err_a + 2^-9 -- the routes differ only in where
    the sum x + residual is rounded; the 1.5 covers the spread between two roundings of the same computation."""
    tables, bad = [], []
    for kind in ("encoder", "decoder"):
        table, b = _layer_table(kind, monkeypatch)
        monkeypatch.undo()
        tables.append(table)
        bad += [f"{kind}: {n}" for n in b]
    text = "\n\n".join(tables)
    print("\n" + text)
    if os.environ.get("RDETR_ACCURACY_OUT"):
        with open(os.environ["RDETR_ACCURACY_OUT"], "w") as f:
            f.write("RelationTransformerEncoderLayer / RelationTransformerDecoderLayer, bf16, .train(), levels (8,10),(4,5),(2,3),(1,2), B = 2, "
                    "24 decoder queries;\nworst |err| / max(1, max|ref|) against the same weights in fp32 with ln_train_fused off\n"
                    + text + "\n")
    assert not bad, f"ln_train_fused less accurate than the torch route: {bad}\n{text}"
