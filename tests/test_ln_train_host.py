"""CPU-only checks of the add + LayerNorm training route's host side: the opt-in switch, the five C entry points declared, bound
and exported with the ABI version unchanged, their argument refusals before any HIP call, the torch fallback of `add_norm` where the
route does not apply, and the shadow tables still complete."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

from relation_detr_amd import _lib, ln_train, options
from relation_detr_amd.transformer import add_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHING = ("rdetr_add_layernorm_train_f32", "rdetr_add_layernorm_train_bf16", "rdetr_add_layernorm_backward_f32",
             "rdetr_add_layernorm_backward_bf16")
WORKSPACE = "rdetr_add_layernorm_backward_workspace_bytes"


def test_ln_train_fused_switch():
    assert options.Options().ln_train_fused is False
    assert options.Options.from_env({}).ln_train_fused is False
    assert options.Options.from_env({"RDETR_LN_TRAIN_FUSED": "1"}).ln_train_fused is True
    assert options.Options.from_env({"RDETR_LN_TRAIN_FUSED": "0"}).ln_train_fused is False
    with pytest.raises(ValueError):
        options.Options.from_env({"RDETR_LN_TRAIN_FUSED": "yes"})


@pytest.mark.parametrize("name", LAUNCHING + (WORKSPACE,))
def test_symbol_is_declared_bound_and_exported(name):
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    ret = "long long" if name == WORKSPACE else "int"
    assert re.search(r"^" + ret + " " + name + r"\s*\(", header, re.M)
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert callable(getattr(_lib.load(), name))


def test_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert "#define RDETR_ABI_VERSION 3" in header
    assert _lib.load().rdetr_abi_version() == 3


def test_workspace_bytes_follow_the_grid_cap():
    ws = _lib.load().rdetr_add_layernorm_backward_workspace_bytes
    part = 2 * 256 * 4                                                     # one [2, 256] fp32 partial
    assert ws(0) == 0 and ws(-3) == 0
    assert ws(1) == part and ws(16) == part and ws(17) == 2 * part
    assert ws(16 * ln_train.MAX_PARTIALS) == ln_train.MAX_PARTIALS * part
    assert ws(16 * ln_train.MAX_PARTIALS + 1) == ln_train.MAX_PARTIALS * part
    assert ws(1 << 40) == ln_train.MAX_PARTIALS * part


@pytest.mark.parametrize("suffix", ["f32", "bf16"])
def test_forward_argument_refusals(suffix):
    fn = getattr(_lib.load(), "rdetr_add_layernorm_train_" + suffix)
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(8)
    a16 = 4 if suffix == "f32" else 8

    def call(x=one, r=one, g=one, b=one, rows=5, C=256, ld=(256, 256, 256), out=one, stats=one):
        return fn(x, r, g, b, rows, C, ld[0], ld[1], ld[2], 1e-5, out, stats, None)
    assert call(x=None, r=None, g=None, b=None, out=None, stats=None, rows=0) == 0        # no rows: nothing launched
    assert call(rows=-1) == -1
    assert call(x=None) == -1 and call(g=None) == -1 and call(b=None) == -1 and call(out=None) == -1 and call(stats=None) == -1
    assert call(ld=(255, 256, 256)) == -1 and call(ld=(256, 255, 256)) == -1 and call(ld=(256, 256, 255)) == -1
    assert call(C=128, ld=(128, 128, 128)) == -2 and call(C=512, ld=(512, 512, 512)) == -2        # no generic-C route
    assert call(x=odd) == -2 and call(r=odd) == -2 and call(g=odd) == -2 and call(b=odd) == -2 and call(out=odd) == -2
    assert call(ld=(256 + a16 // 2, 256, 256)) == -2 and call(ld=(256, 256 + 1, 256)) == -2 and call(ld=(256, 256, 256 + 1)) == -2
    assert call(stats=ctypes.c_void_p(4)) == -2


@pytest.mark.parametrize("suffix", ["f32", "bf16"])
def test_backward_argument_refusals(suffix):
    lib = _lib.load()
    fn = getattr(lib, "rdetr_add_layernorm_backward_" + suffix)
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(8)
    need = lib.rdetr_add_layernorm_backward_workspace_bytes(40)

    def call(dy=one, x=one, r=one, g=one, stats=one, rows=40, C=256, ld=(256, 256, 256), ws=(one, need), dx=one, dg=one, db=one):
        return fn(dy, ld[0], x, ld[1], r, ld[2], g, stats, rows, C, ws[0], ws[1], dx, dg, db, None)
    assert call(dy=None, x=None, r=None, g=None, stats=None, ws=(None, 0), dx=None, dg=None, db=None, rows=0) == 0
    assert call(rows=-1) == -1
    assert call(dy=None) == -1 and call(x=None) == -1 and call(g=None) == -1 and call(stats=None) == -1 and call(dx=None) == -1
    assert call(dg=None) == -1 and call(db=None) == -1                          # the parameter gradients come as a pair
    assert call(ld=(255, 256, 256)) == -1 and call(ld=(256, 255, 256)) == -1 and call(ld=(256, 256, 255)) == -1
    assert call(ws=(None, need)) == -1 and call(ws=(one, need - 1)) == -1 and call(ws=(one, -1)) == -1
    assert call(C=128, ld=(128, 128, 128)) == -2
    assert call(dy=odd) == -2 and call(x=odd) == -2 and call(r=odd) == -2 and call(g=odd) == -2 and call(dx=odd) == -2
    assert call(ws=(odd, need)) == -2 and call(stats=ctypes.c_void_p(4)) == -2
    assert call(ld=(257, 256, 256)) == -2 and call(ld=(256, 257, 256)) == -2 and call(ld=(256, 256, 257)) == -2


def _norm_and_inputs(C=16, dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    norm = torch.nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(C, generator=g))
        norm.bias.copy_(0.1 * torch.randn(C, generator=g))
    norm = norm.to(dtype)
    x = torch.randn(3, 5, C, generator=g).to(dtype).requires_grad_(True)
    r = torch.randn(3, 5, C, generator=g).to(dtype).requires_grad_(True)
    return norm, x, r


@pytest.mark.parametrize("C", [16, 256])
@pytest.mark.parametrize("with_residual", [True, False])
def test_add_norm_on_cpu_keeps_the_torch_route_with_the_option_on(monkeypatch, C, with_residual):
    calls = []
    real = ln_train.AddLayerNormFunction.apply
    monkeypatch.setattr(ln_train.AddLayerNormFunction, "apply", lambda *a: calls.append(1) or real(*a))
    on = dataclasses.replace(options.Options(), ln_train_fused=True)
    norm, x, r = _norm_and_inputs(C)
    res = r if with_residual else None
    got = add_norm(norm, x, res, opts=on)
    want = norm(x + r) if with_residual else norm(x)
    assert torch.equal(got, want) and not calls
    go = torch.randn(got.shape, generator=torch.Generator().manual_seed(4))
    got.backward(go)
    gx, gr, gw, gb = x.grad.clone(), (r.grad.clone() if with_residual else None), norm.weight.grad.clone(), norm.bias.grad.clone()
    for t in (x, r, norm.weight, norm.bias):
        t.grad = None
    want.backward(go)
    assert torch.equal(gx, x.grad) and torch.equal(gw, norm.weight.grad) and torch.equal(gb, norm.bias.grad)
    assert not with_residual or torch.equal(gr, r.grad)
    # the destination form
    out = torch.empty_like(want)
    assert add_norm(norm, x, res, out=out, opts=on) is out and torch.equal(out, want)
    # and the process-level object is what counts without `opts`
    with options.override(ln_train_fused=True):
        assert torch.equal(add_norm(norm, x, res), want) and not calls


def test_supported_refuses_what_the_kernels_do_not_take():
    sup = ln_train.add_layer_norm_train_supported
    w, b = torch.ones(256), torch.zeros(256)
    x = torch.zeros(4, 256)
    assert not sup(x, None, w, b) and not sup(x, x, w, b)                                        # CPU tensors
    assert not sup(torch.zeros(4, 128), None, torch.ones(128), torch.zeros(128))                 # C = 128
    assert not sup(x.bfloat16(), None, w, b) and not sup(x, x.bfloat16(), w, b)                  # mixed dtypes
    assert not sup(x.half(), None, w.half(), b.half())                                           # fp16
    meta = lambda *s, dtype=torch.bfloat16: torch.empty(*s, dtype=dtype, device="meta")          # not a ROCm device either
    assert not sup(meta(4, 256), None, meta(256), meta(256))


def test_no_cpu_path():
    x, w, b = torch.zeros(4, 256), torch.ones(256), torch.zeros(256)
    with pytest.raises(_lib.RdetrError):
        ln_train.add_layer_norm_train(x, None, w, b, 1e-5)
    with pytest.raises(_lib.RdetrError):
        ln_train.add_layer_norm_backward(x, x, None, torch.zeros(4, 2), w)
    with pytest.raises(_lib.RdetrError):
        ln_train.AddLayerNormFunction.apply(x.requires_grad_(True), None, w, b, 1e-5)


def test_package_exports_the_function():
    import relation_detr_amd
    assert relation_detr_amd.AddLayerNormFunction is ln_train.AddLayerNormFunction
    assert "AddLayerNormFunction" in relation_detr_amd.__all__
    assert ln_train.MAX_PARTIALS >= 256 and isinstance(ln_train.MAX_PARTIALS, int)


def test_shadow_tables_still_complete():
    import test_shadow_complete as t
    t.test_every_ops_function_is_classified()
    t.test_every_rdetr_symbol_is_under_the_tripwire_or_excluded()
    t.test_every_options_field_is_switched_in_the_ab_test_or_covered_elsewhere()
