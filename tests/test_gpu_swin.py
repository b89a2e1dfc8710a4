"""The fused shifted-window attention (csrc/attn_win.hip through ``ops.relation_attention(..., window=..., pad=...)``) and the Swin
modules' fused route on the device.

Bounds.  The kernel against the float64 restatement (``backbones.window.window_attention_reference``) on the same bf16 operands:
``|got - ref| <= 2^-7 |ref| + 4e-3``, the bound tests/shadow.py::_attn_cmp holds this kernel family to (P rounded to bf16: 2^-9
relative per term; the output's own rounding: 2^-9; the fixture's logits are O(1), where the absolute term covers exp2's error).
The module routes: the fused route's relative-L2 error against the fp32 torch route may be at most 1.5 x that of the torch route
run in bf16 on the same input -- it rounds P once, like torch's bf16 matmul, and keeps the soft-max in fp32, so it should not be
worse; the margin covers the GEMMs seeing rows in a different order.  Nothing here runs under ``Shadow``: tests/shadow.py does
not know the windowed mode."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard
import relation_detr_amd
from relation_detr_amd import _lib, ops
from relation_detr_amd.backbones import SwinTransformerBackbone
from relation_detr_amd.backbones import window as wgeo
from test_swin_host import CASES, attention_module, case_of, small_net

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SYMBOL = "rdetr_window_attention_bf16"


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_swin.npz")


@pytest.fixture(scope="module")
def g16_net(golden):
    return golden("g16_swin_net.npz")


def assert_close(got, ref, what):
    """got bf16 [B, L, C] from the kernel, ref float64 on the host."""
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 4e-3
    print(f"{what}: max error {err.max().item():.3e}, largest error / bound {(err / bound).max().item():.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (what, err.max().item(), (err / bound).max().item())


def operands(c, table_dtype=torch.float32):
    """The qkv GEMM's bf16 output on the unpadded map, the table and the pad rows of a fixture case, on the device."""
    H, W, wh, ww, sh, sw, B, C, heads = (int(v) for v in c["cfg"])
    m = attention_module(c, BF16).to(DEV)
    x = torch.from_numpy(c["x"]).to(DEV, BF16).reshape(B, H * W, C)
    with torch.no_grad():
        qkv = m.qkv(x)
    row = m.qkv.bias.detach()
    window = (H, W, wh, ww, *wgeo.effective_shift(H, W, wh, ww, sh, sw))
    return qkv, torch.from_numpy(c["table"]).to(DEV, table_dtype), (row[C:2 * C], row[2 * C:]), window, heads, C


def call(qkv, table, pad, window, heads, C):
    return ops.relation_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, bias=table, window=window, pad=pad)


def reference(qkv, table, pad, window, heads, C):
    return wgeo.window_attention_reference(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, table, window, pad=pad)


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", CASES)
def test_kernel_against_float64_on_the_fixture(g16, name):
    args = operands(case_of(g16, name))
    got = call(*args)
    assert got.dtype == BF16 and got.shape == args[0][..., :args[-1]].shape and got.is_contiguous()
    assert_close(got, reference(*args), name)


@pytest.mark.parametrize("name", ["w7_s3_9x17", "w12_s6_13x25", "w3x5_s1x2_7x11"])
@pytest.mark.parametrize("table_dtype", [torch.float32, BF16])
@pytest.mark.parametrize("with_pad", [True, False])
def test_table_dtypes_pad_and_a_side_stream(g16, name, table_dtype, with_pad):
    qkv, table, pad, window, heads, C = operands(case_of(g16, name), table_dtype)
    pad = pad if with_pad else None
    ref = reference(qkv, table, pad, window, heads, C)
    got = call(qkv, table, pad, window, heads, C)
    assert_close(got, ref, f"{name} table {table_dtype} pad {with_pad}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = call(qkv, table, pad, window, heads, C)
    side.synchronize()
    assert torch.equal(again, got)


def test_column_views_and_separate_tensors_give_the_same_bits(g16):
    qkv, table, pad, window, heads, C = operands(case_of(g16, "w7_s3_9x17"))
    got = call(qkv, table, pad, window, heads, C)
    q, k, v = (qkv[..., i * C:(i + 1) * C].contiguous() for i in range(3))
    assert q.stride(1) == C and qkv[..., :C].stride(1) == 3 * C
    assert torch.equal(ops.relation_attention(q, k, v, heads, bias=table, window=window, pad=pad), got)
    assert torch.equal(ops.relation_attention(q, k, v, heads, bias=table, window=window, pad=tuple(p.clone() for p in pad)), got)


def test_padding_tokens_are_keys_with_the_pad_rows():
    """One 7 x 7 window over a 5 x 6 map (19 padding tokens, 30 real ones; 30 is no multiple of 16) and a shifted 9 x 10 map, with
    pad rows no real token resembles: v_pad = 4 everywhere, k_pad aligned with the mean query.  Padding treated as masked or as zero
    misses the bound by far, which the test shows for the zero case before it holds the kernel to the reference."""
    g = torch.Generator().manual_seed(5)
    heads, C = 2, 64
    for (H, W, sh, sw) in ((5, 6, 0, 0), (9, 10, 3, 3)):
        qkv = torch.randn(2, H * W, 3 * C, generator=g).to(DEV, BF16)
        table = (torch.randn(13 * 13, heads, generator=g) * 0.5).to(DEV)
        k_pad = (qkv[..., :C].float().mean((0, 1)) * 2.0).to(BF16).contiguous()
        v_pad = torch.full((C,), 4.0, device=DEV, dtype=BF16)
        window = (H, W, 7, 7, sh, sw)
        ref = reference(qkv, table, (k_pad, v_pad), window, heads, C)
        zero = reference(qkv, table, None, window, heads, C)
        far = (ref - zero).abs() > 8 * (2.0 ** -7 * ref.abs() + 4e-3)
        assert far.float().mean().item() > 0.5                           # most outputs see the padding keys
        assert_close(call(qkv, table, (k_pad, v_pad), window, heads, C), ref, f"distinctive pad rows {H}x{W}")
        assert_close(call(qkv, table, None, window, heads, C), zero, f"no pad rows {H}x{W}")


def test_refusals_and_the_empty_problem():
    qkv = torch.zeros(1, 35, 192, device=DEV, dtype=BF16)
    table = torch.zeros(169, 2, device=DEV)
    lib = _lib.load()

    def status(D=32, wh=7, ww=7, sh=0, sw=0, B=1, H=5, W=7, table_ptr=None):
        out = torch.empty(1, 35, 64, device=DEV, dtype=BF16)
        return lib.rdetr_window_attention_bf16(qkv.data_ptr(), qkv.data_ptr() + 128, qkv.data_ptr() + 256, 192, 192, 192, None, None,
                                               table.data_ptr() if table_ptr is None else table_ptr, 0, B, 2, D, H, W, wh, ww, sh, sw,
                                               0.17, out.data_ptr(), 64, torch.cuda.current_stream().cuda_stream)
    assert status() == 0
    assert status(D=16) == -2 and status(wh=13, ww=12) == -2              # head dim, more than 144 tokens
    assert status(wh=0) == -1 and status(sh=7) == -1 and status(sw=7) == -1 and status(sh=-1) == -1
    assert status(B=0) == 0 and status(H=0) == 0                           # the empty problem launches nothing
    assert status(table_ptr=table.data_ptr() + 2) == -2
    with pytest.raises(_lib.RdetrError, match="unsupported|UNSUPPORTED|status -2"):
        ops.relation_attention(torch.zeros(1, 35, 32, device=DEV, dtype=BF16), torch.zeros(1, 35, 32, device=DEV, dtype=BF16),
                               torch.zeros(1, 35, 32, device=DEV, dtype=BF16), 2, bias=table, window=(5, 7, 7, 7, 0, 0))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- write set
def test_write_set_under_guard_bands(g16, monkeypatch):
    c = case_of(g16, "w12_s6_13x25")
    qkv, table, pad, window, heads, C = operands(c)
    ref = reference(qkv, table, pad, window, heads, C)
    g = guard.guard(monkeypatch)
    held = lambda t: torch.empty(t.shape, dtype=t.dtype, device=DEV).copy_(t)                              # noqa: E731
    qkv_g, table_g, k_pad, v_pad = held(qkv), held(table), held(pad[0]), held(pad[1])
    q, k, v = (held(qkv[..., i * C:(i + 1) * C].contiguous()) for i in range(3))
    inputs = (qkv_g, table_g, k_pad, v_pad, q, k, v)
    before = [t.clone() for t in inputs]
    n = len(g.allocations)
    got_views = call(qkv_g, table_g, (k_pad, v_pad), window, heads, C)
    got_split = ops.relation_attention(q, k, v, heads, bias=table_g, window=window, pad=(k_pad, v_pad))
    torch.cuda.synchronize()
    assert len(g.allocations) - n == 2                                     # the two results, nothing else
    assert g.check() == []
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(inputs, before))       # inputs bit-identical
    for got in (got_views, got_split):
        a = g.of(got)
        assert a is not None and a.span == got.numel() * 2                 # rows [0, H * W) of every image, all of them written
        assert_close(got, ref, "guarded")
    assert torch.equal(got_views, got_split)


# ---------------------------------------------------------------------------------------------------------------- the modules
def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_fused_route_of_the_network_against_the_torch_route(g16_net):
    x = torch.from_numpy(g16_net["net.x"]).to(DEV)
    net32 = small_net(g16_net, torch.float32).to(DEV)
    fused = small_net(g16_net, BF16).to(DEV).requires_grad_(False)
    plain = small_net(g16_net, BF16, fused=False).to(DEV).requires_grad_(False)
    with torch.no_grad():
        want = net32.stages_torch(x)
        assert all(blk.attn.takes_fused_route(torch.zeros(1, 9, 17, blk.attn.qkv.in_features, device=DEV, dtype=BF16))
                   for stage in (fused.features[1], fused.features[3]) for blk in stage)
        got_fused = fused(x.to(BF16))
        got_plain = plain(x.to(BF16))
        assert all(torch.equal(a, b) for a, b in zip(plain.stages_torch(x.to(BF16)), got_plain))
    for name, w, f, p in zip(("features.1", "features.3"), want, got_fused, got_plain):
        e_fused, e_plain = rel_l2(f, w), rel_l2(p, w)
        print(f"{name}: relative L2 against fp32 -- torch bf16 route {e_plain:.4e}, fused route {e_fused:.4e}")
        assert e_fused <= 1.5 * e_plain, (name, e_fused, e_plain)


class Counting:
    """Stands in for the loaded library: counts the calls of every symbol and passes them on."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("rdetr_"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_training_step_routes_the_frozen_stage_through_the_kernel(monkeypatch):
    kw = dict(embed_dim=64, depths=(2, 2), num_heads=(2, 4), stochastic_depth_prob=0.0)
    torch.manual_seed(3)
    models = {f: SwinTransformerBackbone("swin_t", return_indices=(0, 1), freeze_indices=(0,), fused=f, **kw).to(DEV).train() for f in (True, False)}
    with torch.no_grad():
        for p in models[True].parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn_like(p) * p[0].numel() ** -0.5)
    models[False].load_state_dict(models[True].state_dict())
    exact = SwinTransformerBackbone("swin_t", return_indices=(0, 1), freeze_indices=(0,), fused=False, **kw).to(DEV).train()
    exact.load_state_dict(models[True].state_dict())
    x = torch.randn(2, 3, 36, 68, device=DEV)
    counting = Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: counting)

    def grads(model, autocast):
        before = counting.calls.get(SYMBOL, 0)
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF16, enabled=autocast):
            out = model(x)
            loss = sum(o.float().square().mean() for o in out.values())
        loss.backward()
        named = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
        assert named and all(g is not None for g in named.values()) and all(n.startswith("features.3.") for n in named)
        return torch.cat([g.flatten().double() for g in named.values()]), counting.calls.get(SYMBOL, 0) - before

    want, n_exact = grads(exact, False)
    got_fused, n_fused = grads(models[True], True)
    got_plain, n_plain = grads(models[False], True)
    assert (n_exact, n_fused, n_plain) == (0, 2, 0)                        # the two blocks of stage 0, and nothing of stage 1
    e_fused, e_plain = rel_l2(got_fused, want), rel_l2(got_plain, want)
    print(f"gradients of stage 1: relative L2 against fp32 -- torch route under autocast {e_plain:.4e}, fused stage 0 {e_fused:.4e}")
    assert e_fused <= 1.5 * e_plain, (e_fused, e_plain)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        before = counting.calls.get(SYMBOL, 0)
        models[True].eval()(x)
        assert counting.calls[SYMBOL] - before == 4                        # without gradients every attention qualifies
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        models[True](x)
        assert counting.calls[SYMBOL] - before == 4


def test_detector_with_the_swin_backbone_end_to_end(monkeypatch):
    torch.manual_seed(45)
    model = relation_detr_amd.relation_detr_swin_l(
        num_classes=11, num_queries=30, hybrid_num_proposals=30, enc_layers=2, dec_layers=2, d_ffn=64, denoising_nums=6, min_size=64,
        max_size=100, num_select=10, arch="swin_t", backbone_kwargs=dict(embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8)))
    assert isinstance(model.backbone, SwinTransformerBackbone) and model.backbone.return_layers == ["features.3", "features.5", "features.7"]
    assert model.backbone.freeze_indices == (0,) and [c[0].in_channels for c in model.neck.convs][:3] == [64, 128, 256]
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(47)
    images = [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g).to(DEV) for h, w in ((70, 100), (96, 71))]
    with torch.no_grad():
        dets, tensor = model(images)
    assert tuple(tensor.shape) == (2, 10, 6) and bool(torch.isfinite(tensor).all()) and len(dets) == 2
    for d in dets:
        assert set(d) == {"scores", "labels", "boxes"} and tuple(d["boxes"].shape) == (10, 4) and d["labels"].dtype == torch.int64
    # the backbone of that detector under bf16 autocast: every attention through the kernel, and no farther from the fp32 maps
    # than 1.5 x the torch route under the same autocast (the rule of the module test above)
    counting = Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: counting)
    batch = torch.randn(2, 3, 96, 128, device=DEV)
    with torch.no_grad():
        want = model.backbone(batch)
        assert SYMBOL not in counting.calls
        with torch.autocast("cuda", dtype=BF16):
            got = model.backbone(batch)
            assert counting.calls[SYMBOL] == 8
            plain = model.backbone.forward_torch(batch)
    assert counting.calls[SYMBOL] == 8 and list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].is_contiguous()
        assert rel_l2(got[k], want[k]) <= 1.5 * rel_l2(plain[k], want[k]), k
