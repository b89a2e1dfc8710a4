"""CPU-only checks of the mixed-precision training routes' host side (relation_detr_amd/amp_train.py): the five C entry points
declared, bound and exported with the ABI version unchanged, their argument refusals before any HIP call, the pure dtype / shape rule
of the mixed add + LayerNorm route, no CPU path, the unchanged torch route of `add_norm` / `feed_forward` off the device, and the
set of `Options` fields as it was."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

from relation_detr_amd import _lib, amp_train, options
from relation_detr_amd.transformer import add_norm, feed_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rdetr_add_layernorm_train_mixed", "rdetr_add_layernorm_backward_mixed", "rdetr_ffn_k256_pack_f32",
           "rdetr_ffn_k256_train_xf32_bf16", "rdetr_ffn_k256_backward_dxf32_bf16")
OPTION_FIELDS = {
    "linear_k256", "ffn_fused", "ffn_ln", "ffn_train_fused", "ln_train_fused", "ln_pos", "decoder_ln_pos", "decoder_entry", "decoder_tail",
    "decoder_value_batched", "box_head", "rel_fused", "pyramid_points", "topk", "detections_kernel", "mask_in_kernel", "value_head_major",
    "value_proj_hm", "merged_proj", "proj_ln", "encoder_proj", "msda_train_fused", "msda_train_head_major", "attn_train_fused",
    "rel_train_fused"}
F32, BF, HALF = torch.float32, torch.bfloat16, torch.float16
ONE, ODD = ctypes.c_void_p(16), ctypes.c_void_p(8)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_bound_and_exported(name):
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert re.search(r"^int " + name + r"\s*\(", header, re.M)
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert callable(getattr(_lib.load(), name))


def test_abi_version_and_option_fields_are_unchanged():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert "#define RDETR_ABI_VERSION 3" in header
    assert _lib.load().rdetr_abi_version() == 3
    assert {f.name for f in dataclasses.fields(options.Options)} == OPTION_FIELDS
    assert options.Options().ln_train_fused is False and options.Options().ffn_train_fused is False


def test_norm_rule_accepts_what_autocast_hands_over():
    """The calls a bf16-autocast step over fp32 parameters makes (x, residual) -- all with fp32 parameters and an fp32 result."""
    ok = amp_train.mixed_norm_operands_ok
    w, b = torch.ones(256), torch.zeros(256)
    x32, xbf = torch.zeros(2, 5, 256), torch.zeros(2, 5, 256, dtype=BF)
    assert ok(x32, xbf, w, b, True)                          # a layer norm: the fp32 residual stream + a sublayer's bf16 linear output
    assert ok(xbf, x32, w, b, True)                          # the MSDA module's output stage: bf16 output_proj + the fp32 stream
    assert ok(x32, None, w, b, True) and ok(xbf, None, w, b, True)       # decoder.norm, enc_output_norm, memory_fusion[3]
    assert ok(xbf, xbf, w, b, True)
    # outside autocast only "everything fp32" is left to the same-dtype route
    assert ok(x32, xbf, w, b, False) and ok(xbf, None, w, b, False)
    assert not ok(x32, None, w, b, False) and not ok(x32, x32, w, b, False)


def test_norm_rule_refusals():
    ok = amp_train.mixed_norm_operands_ok
    w, b = torch.ones(256), torch.zeros(256)
    x = torch.zeros(4, 256)
    assert not ok(x.to(HALF), None, w, b, True) and not ok(x, x.to(HALF), w, b, True)                 # fp16
    assert not ok(torch.zeros(4, 255), None, torch.ones(255), torch.zeros(255), True)               # 255 channels
    assert not ok(x, None, torch.ones(255), torch.zeros(255), True)
    assert not ok(x, x.to(BF), w.to(BF), b.to(BF), True) and not ok(x, None, w, b.to(BF), True)       # bf16 parameters
    assert not ok(x, torch.zeros(2, 256, dtype=BF), w, b, True)                                     # a residual of another shape
    assert not ok(x, torch.zeros(4, 1, 256, dtype=BF), w, b, True)
    assert not ok(x, None, None, None, True) and not ok(None, None, w, b, True)
    # the device form refuses CPU tensors whatever their dtypes
    assert not amp_train.add_layer_norm_mixed_supported(x, x.to(BF), w, b)
    assert not amp_train.ffn_mixed_supported(torch.zeros(4, 256), torch.zeros(64, 256), torch.zeros(64), torch.zeros(256, 64), b)


def test_autocast_probe_is_false_outside_autocast():
    assert amp_train.autocast_bf16_active() is False


def test_no_cpu_path():
    x, w, b = torch.zeros(4, 256), torch.ones(256), torch.zeros(256)
    w1, b1, w2 = torch.zeros(64, 256), torch.zeros(64), torch.zeros(256, 64)
    with pytest.raises(_lib.RdetrError):
        amp_train.add_layer_norm_mixed_train(x, x.to(BF), w, b, 1e-5)
    with pytest.raises(_lib.RdetrError):
        amp_train.add_layer_norm_mixed_backward(x, x, x.to(BF), torch.zeros(4, 2), w)
    with pytest.raises(_lib.RdetrError):
        amp_train.AddLayerNormMixedFunction.apply(x.clone().requires_grad_(True), x.to(BF), w, b, 1e-5)
    with pytest.raises(_lib.RdetrError):
        amp_train.ffn_pack_f32(w1, w2, b1, b)
    with pytest.raises(_lib.RdetrError):
        amp_train.ffn_mixed_train(x, w1, b1, w2, b)
    with pytest.raises(_lib.RdetrError):
        amp_train.ffn_mixed_backward(x.to(BF), torch.zeros(4, 64, dtype=BF), w1, w2)
    with pytest.raises(_lib.RdetrError):
        amp_train.FeedForwardMixedFunction.apply(x.clone().requires_grad_(True), w1, b1, w2, b)


def test_package_exports_the_functions():
    import relation_detr_amd
    for name in ("AddLayerNormMixedFunction", "FeedForwardMixedFunction"):
        assert getattr(relation_detr_amd, name) is getattr(amp_train, name) and name in relation_detr_amd.__all__


def test_cpu_calls_keep_the_torch_route_with_the_switches_on(monkeypatch):
    calls = []
    monkeypatch.setattr(amp_train.AddLayerNormMixedFunction, "apply", lambda *a: calls.append("ln"))
    monkeypatch.setattr(amp_train.FeedForwardMixedFunction, "apply", lambda *a: calls.append("ffn"))
    on = dataclasses.replace(options.Options(), ln_train_fused=True, ffn_train_fused=True)
    g = torch.Generator().manual_seed(0)
    norm, l1, l2 = torch.nn.LayerNorm(256), torch.nn.Linear(256, 64), torch.nn.Linear(64, 256)
    x = torch.randn(3, 5, 256, generator=g).requires_grad_(True)
    r = torch.randn(3, 5, 256, generator=g).to(BF)
    with torch.autocast("cpu", dtype=BF):
        assert torch.equal(add_norm(norm, x, r, opts=on), norm(x + r))
        assert torch.equal(feed_forward(l1, l2, x, on), l2(torch.relu(l1(x))))
    assert torch.equal(add_norm(norm, x, r.float(), opts=on), norm(x + r.float()))
    assert not calls


# ------------------------------------------------------------------------------------------- argument refusals (no HIP call)
def test_layernorm_forward_refusals():
    fn = _lib.load().rdetr_add_layernorm_train_mixed

    def call(x=ONE, xb=0, ldx=256, r=ONE, rb=1, ldr=256, g=ONE, b=ONE, rows=5, C=256, out=ONE, ldo=256, stats=ONE):
        return fn(x, xb, ldx, r, rb, ldr, g, b, rows, C, 1e-5, out, ldo, stats, None)
    assert call(x=None, r=None, g=None, b=None, out=None, stats=None, rows=0) == 0        # no rows: nothing launched
    assert call(rows=-1) == -1
    assert call(x=None) == -1 and call(g=None) == -1 and call(b=None) == -1 and call(out=None) == -1 and call(stats=None) == -1
    assert call(ldx=255) == -1 and call(ldr=255) == -1 and call(ldo=255) == -1
    assert call(C=128, ldx=128, ldr=128, ldo=128) == -2 and call(C=512, ldx=512, ldr=512, ldo=512) == -2
    assert call(x=ODD) == -2 and call(r=ODD) == -2 and call(g=ODD) == -2 and call(b=ODD) == -2 and call(out=ODD) == -2
    # each operand on the 16-byte grid of its OWN type: 4 fp32 elements, 8 bf16 elements
    assert call(ldx=258) == -2 and call(xb=1, ldx=260) == -2 and call(ldr=260) == -2 and call(rb=0, ldr=258) == -2 and call(ldo=258) == -2
    assert call(stats=ctypes.c_void_p(4)) == -2


def test_layernorm_backward_refusals():
    lib = _lib.load()
    fn = lib.rdetr_add_layernorm_backward_mixed
    need = lib.rdetr_add_layernorm_backward_workspace_bytes(40)

    def call(dy=ONE, lddy=256, x=ONE, xb=0, ldx=256, r=ONE, rb=1, ldr=256, g=ONE, stats=ONE, rows=40, C=256, ws=(ONE, need), dx=ONE,
             dxb=ONE, dg=ONE, db=ONE):
        return fn(dy, lddy, x, xb, ldx, r, rb, ldr, g, stats, rows, C, ws[0], ws[1], dx, dxb, dg, db, None)
    assert call(dy=None, x=None, r=None, g=None, stats=None, ws=(None, 0), dx=None, dxb=None, dg=None, db=None, rows=0) == 0
    assert call(rows=-1) == -1
    assert call(dy=None) == -1 and call(x=None) == -1 and call(g=None) == -1 and call(stats=None) == -1
    assert call(dg=None) == -1 and call(db=None) == -1                          # the parameter gradients come as a pair
    # a gradient tensor for every operand type that occurs
    assert call(dx=None) == -1 and call(dxb=None) == -1                         # x fp32, residual bf16: both
    assert call(xb=0, rb=0, dxb=None, dx=None) == -1 and call(xb=1, rb=1, dx=None, dxb=None) == -1
    assert call(xb=1, r=None, dxb=None) == -1 and call(xb=0, r=None, dx=None) == -1
    assert call(lddy=255) == -1 and call(ldx=255) == -1 and call(ldr=255) == -1
    assert call(ws=(None, need)) == -1 and call(ws=(ONE, need - 1)) == -1 and call(ws=(ONE, -1)) == -1
    assert call(C=128, lddy=128, ldx=128, ldr=128) == -2
    assert call(dy=ODD) == -2 and call(x=ODD) == -2 and call(r=ODD) == -2 and call(g=ODD) == -2 and call(dx=ODD) == -2 and call(dxb=ODD) == -2
    assert call(ws=(ODD, need)) == -2 and call(stats=ctypes.c_void_p(4)) == -2
    assert call(lddy=258) == -2 and call(ldx=258) == -2 and call(ldr=260) == -2 and call(xb=1, ldx=260) == -2


def test_pack_refusals():
    fn = _lib.load().rdetr_ffn_k256_pack_f32

    def call(w1=ONE, s1=(256, 1), w2=ONE, s2=(128, 1), b1=ONE, b2=ONE, F=128, packed=ONE, biases=ONE):
        return fn(w1, s1[0], s1[1], w2, s2[0], s2[1], b1, b2, F, packed, biases, None)
    assert call(F=0) == -1 and call(F=-64) == -1
    assert call(F=100) == -2 and call(F=4160) == -2
    assert call(w1=None) == -1 and call(w2=None) == -1 and call(packed=None) == -1
    assert call(s1=(0, 1)) == -1 and call(s1=(256, 0)) == -1 and call(s2=(-1, 1)) == -1 and call(s2=(128, 0)) == -1
    assert call(b1=None) == -1 and call(b2=None) == -1 and call(biases=None) == -1 and call(b1=None, b2=None) == -1   # all or none
    assert call(packed=ODD) == -2 and call(w1=ctypes.c_void_p(18)) == -2 and call(w2=ctypes.c_void_p(18)) == -2
    assert call(b1=ctypes.c_void_p(18)) == -2 and call(biases=ctypes.c_void_p(17)) == -2


def test_ffn_forward_refusals():
    fn = _lib.load().rdetr_ffn_k256_train_xf32_bf16

    def call(x=ONE, ldx=256, packed=ONE, b1=ONE, b2=ONE, M=300, F=128, out=ONE, ldo=256, hid=ONE, ldh=None, xlp=ONE, ldxl=256):
        return fn(x, ldx, packed, b1, b2, M, F, out, ldo, hid, F if ldh is None else ldh, xlp, ldxl, None)
    assert call(M=0) == 0
    assert call(M=-1) == -1 and call(F=0) == -1
    assert call(ldx=255) == -1 and call(ldo=255) == -1 and call(ldh=127) == -1 and call(ldxl=255) == -1
    assert call(x=None) == -1 and call(packed=None) == -1 and call(b1=None) == -1 and call(b2=None) == -1 and call(out=None) == -1
    assert call(hid=None) == -1 and call(xlp=None) == -1
    assert call(F=100) == -2 and call(F=4160) == -2
    assert call(ldx=258) == -2 and call(ldo=260) == -2 and call(ldh=132) == -2 and call(ldxl=260) == -2
    assert call(x=ODD) == -2 and call(packed=ODD) == -2 and call(out=ODD) == -2 and call(hid=ODD) == -2 and call(xlp=ODD) == -2
    assert call(M=1 << 20, F=2048) == -2                                        # H beyond 32-bit byte offsets


def test_ffn_backward_refusals():
    fn = _lib.load().rdetr_ffn_k256_backward_dxf32_bf16

    def call(dy=ONE, lddy=256, packed=ONE, hid=ONE, ldh=None, M=300, F=128, dh=ONE, ldd=None, dx=ONE, lddx=256):
        return fn(dy, lddy, packed, hid, F if ldh is None else ldh, M, F, dh, F if ldd is None else ldd, dx, lddx, None)
    assert call(M=0) == 0
    assert call(M=-1) == -1 and call(F=0) == -1
    assert call(lddy=255) == -1 and call(lddx=255) == -1 and call(ldh=127) == -1 and call(ldd=127) == -1
    assert call(dy=None) == -1 and call(packed=None) == -1 and call(hid=None) == -1 and call(dh=None) == -1 and call(dx=None) == -1
    assert call(F=100) == -2 and call(F=4160) == -2
    assert call(lddy=260) == -2 and call(lddx=258) == -2 and call(ldh=132) == -2 and call(ldd=132) == -2
    assert call(dy=ODD) == -2 and call(packed=ODD) == -2 and call(hid=ODD) == -2 and call(dh=ODD) == -2 and call(dx=ODD) == -2
    assert call(M=1 << 20, F=2048) == -2
