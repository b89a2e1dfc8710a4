"""GPU checks of the neck kernels (csrc/neck.hip) and of the modules on top (relation_detr_amd/neck.py, RelationDETR).

GroupNorm bound, forward and backward, per tensor: the yardstick is the error of torch's own fp32 CPU kernel against float64 on the
same operands, measured here; the kernel may err 4 x max(that, 2^-23 max|ref|): the reference implementation's own rounding with a
margin for a different summation tree.  bf16: one more rounding of the output, 2^-8 |ref| on top, on bf16-rounded operands.
Masks and counts are exact.  Position encoding: 5e-6 (the bound of the project's other sine features for arguments of this
construction) against float64 sin / cos of the fp32 argument, which the test rebuilds on the CPU with the same single operations."""
import copy
from functools import partial

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

from conftest import load_golden
from helpers import synthetic_state_dict
from relation_detr_amd import neck
from relation_detr_amd.neck import ChannelMapper, PositionEmbeddingSine, PyramidBuilder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
T = torch.from_numpy
EPS = 1e-5
POS_TOL = 5e-6
G12_SIZES = ((12, 20), (6, 10), (3, 5), (2, 3))
R50_SIZES = ((100, 168), (50, 84), (25, 42), (13, 21))
# name -> (B, C, G, level sizes, input mean)
GN_CASES = {
    "g12 pyramid, C 32 / G 8": (2, 32, 8, G12_SIZES, 0.0),
    "g12 pyramid, C 256 / G 32": (2, 256, 32, G12_SIZES, 0.0),
    "five levels down to (1, 2), B 3": (3, 32, 4, G12_SIZES + ((1, 2),), 0.0),
    "R50 sizes, B 1: groups split over many workgroups": (1, 256, 32, R50_SIZES, 0.0),
    "mean 100, std 1": (2, 64, 8, ((25, 42), (13, 21)), 100.0),
}


def gn_operands(name, dtype=F32):
    B, C, G, sizes, mean = GN_CASES[name]
    g = torch.Generator().manual_seed(len(name))
    xs = [(torch.randn(B, C, h, w, generator=g) + mean).to(dtype) for h, w in sizes]
    ws = [1.0 + 0.3 * torch.randn(C, generator=g) for _ in sizes]
    bs = [0.3 * torch.randn(C, generator=g) for _ in sizes]
    gos = [torch.randn(B, C, h, w, generator=g).to(dtype) for h, w in sizes]
    return G, xs, ws, bs, gos


def cpu_group_norm(xs, ws, bs, gos, G, dtype):
    """Outputs and gradients (dx, dgamma, dbeta per level) of torch's CPU GroupNorm in ``dtype`` on the given operands."""
    out = []
    for x, w, b, go in zip(xs, ws, bs, gos):
        x, w, b = (t.detach().to(dtype).requires_grad_() for t in (x, w, b))
        y = F.group_norm(x, G, w, b, EPS)
        y.backward(go.to(dtype))
        out.append((y.detach(), x.grad, w.grad, b.grad))
    return out


def yardstick_bound(ref64: torch.Tensor, cpu32: torch.Tensor) -> float:
    own = float((cpu32.to(F64) - ref64).abs().max())
    return 4.0 * max(own, 2.0 ** -23 * float(ref64.abs().max()))


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_neck.npz")


@pytest.fixture(scope="module")
def gn_refs():
    """name -> (operands, float64 results, fp32 CPU results), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            G, xs, ws, bs, gos = gn_operands(name)
            cache[name] = ((G, xs, ws, bs, gos), cpu_group_norm(xs, ws, bs, gos, G, F64), cpu_group_norm(xs, ws, bs, gos, G, F32))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(GN_CASES))
def test_group_norm_forward_and_backward_fp32(gn_refs, name):
    (G, xs, ws, bs, gos), ref64, cpu32 = gn_refs(name)
    dx_ = [x.to(DEV).requires_grad_() for x in xs]
    dw_ = [w.to(DEV).requires_grad_() for w in ws]
    db_ = [b.to(DEV).requires_grad_() for b in bs]
    ys = neck.group_norm_levels(dx_, dw_, db_, G, EPS)
    torch.autograd.backward(ys, [go.to(DEV) for go in gos])
    for l, y in enumerate(ys):
        got = (y.detach(), dx_[l].grad, dw_[l].grad, db_[l].grad)
        for what, g_, r64, c32 in zip(("y", "dx", "dgamma", "dbeta"), got, ref64[l], cpu32[l]):
            err, bound = float((g_.cpu().to(F64) - r64).abs().max()), yardstick_bound(r64, c32)
            print(f"{name} level {l} {what}: err {err:.3e} bound {bound:.3e} (torch fp32 CPU {float((c32.to(F64) - r64).abs().max()):.3e})")
            assert err <= bound, (name, l, what, err, bound)
    # the statistics kept for the backward, and a second call: the same bits
    ys2, mean, rstd = neck.group_norm_levels_forward([x.detach() for x in dx_], dw_, db_, G, EPS)
    assert all(torch.equal(a, b.detach()) for a, b in zip(ys2, ys))
    B, C = xs[0].shape[:2]
    for l, x in enumerate(xs):
        m64 = x.to(F64).view(B, G, -1).mean(-1)
        assert float((mean[l].cpu().to(F64) - m64).abs().max()) <= 4 * 2.0 ** -23 * max(1.0, float(m64.abs().max()))
    dxs, dgamma, dbeta = neck.group_norm_levels_backward([go.to(DEV) for go in gos], [x.detach() for x in dx_], dw_, mean, rstd, G)
    for l in range(len(xs)):
        assert torch.equal(dxs[l], dx_[l].grad) and torch.equal(dgamma[l], dw_[l].grad) and torch.equal(dbeta[l], db_[l].grad)


@pytest.mark.parametrize("name,params_bf16", [("g12 pyramid, C 32 / G 8", True), ("R50 sizes, B 1: groups split over many workgroups", False),
                                              ("five levels down to (1, 2), B 3", False)])
def test_group_norm_bf16(name, params_bf16):
    G, xs, ws, bs, gos = gn_operands(name, BF16)
    if params_bf16:
        ws, bs = [w.to(BF16) for w in ws], [b.to(BF16) for b in bs]
    ref64 = cpu_group_norm(xs, ws, bs, gos, G, F64)
    cpu32 = cpu_group_norm(xs, ws, bs, gos, G, F32)
    dx_ = [x.to(DEV).requires_grad_() for x in xs]
    dw_ = [w.to(DEV).requires_grad_() for w in ws]
    db_ = [b.to(DEV).requires_grad_() for b in bs]
    ys = neck.group_norm_levels(dx_, dw_, db_, G, EPS)
    assert all(y.dtype == BF16 for y in ys)
    torch.autograd.backward(ys, [go.to(DEV) for go in gos])
    for l, y in enumerate(ys):
        assert dw_[l].grad.dtype == ws[l].dtype and dx_[l].grad.dtype == BF16
        for what, g_, r64, c32, rounded in (("y", y.detach(), ref64[l][0], cpu32[l][0], True), ("dx", dx_[l].grad, ref64[l][1], cpu32[l][1], True),
                                            ("dgamma", dw_[l].grad, ref64[l][2], cpu32[l][2], params_bf16),
                                            ("dbeta", db_[l].grad, ref64[l][3], cpu32[l][3], params_bf16)):
            err = (g_.cpu().to(F64) - r64).abs()
            bound = yardstick_bound(r64, c32) + (2.0 ** -8 * r64.abs() if rounded else 0.0)
            print(f"bf16 {name} level {l} {what}: err {float(err.max()):.3e} fp32 part of the bound {yardstick_bound(r64, c32):.3e}")
            assert bool((err <= bound).all()), (name, l, what, float(err.max()))


def golden_mapper(z, fused, num_outs=4, prefix="sd."):
    m = ChannelMapper([16, 24, 40], 32, num_outs, norm_layer=partial(nn.GroupNorm, 8), fused=fused)
    m.load_state_dict({k[len(prefix):]: T(v) for k, v in z.items() if k.startswith(prefix)})
    return m


def test_fused_channel_mapper_against_g12(g12):
    """Outputs and gradients of the fused mapper against float64 (the torch route on the CPU), the recorded fp32 results as yardstick."""
    ref = golden_mapper(g12, False).double()
    xs64 = [T(g12[f"x{i}"]).double().requires_grad_() for i in range(3)]
    ys64 = ref(xs64)
    sum((y * T(g12[f"go{i}"]).double()).sum() for i, y in enumerate(ys64)).backward()
    m = golden_mapper(g12, True).to(DEV)
    xs = [T(g12[f"x{i}"]).to(DEV).requires_grad_() for i in range(3)]
    assert m.takes_fused_route(xs)
    ys = m({str(i): x for i, x in enumerate(xs)})
    sum((y * T(g12[f"go{i}"]).to(DEV)).sum() for i, y in enumerate(ys)).backward()
    checks = [(f"y{i}", ys[i].detach(), ys64[i].detach(), g12[f"y{i}"]) for i in range(4)]
    checks += [(f"gx{i}", xs[i].grad, xs64[i].grad, g12[f"gx{i}"]) for i in range(3)]
    checks += [(f"gsd.{k}", p.grad, dict(ref.named_parameters())[k].grad, g12[f"gsd.{k}"]) for k, p in m.named_parameters()]
    for what, got, r64, rec in checks:
        err, bound = float((got.cpu().to(F64) - r64).abs().max()), yardstick_bound(r64, T(rec))
        print(f"fused ChannelMapper {what}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, err, bound)
    m5 = golden_mapper(g12, True, 5, "sd5.").to(DEV)                            # an extra level behind the extra level: a second call
    ref5 = golden_mapper(g12, False, 5, "sd5.").double()
    with torch.no_grad():
        y5, r5 = m5([x.detach() for x in xs]), ref5([x.detach() for x in xs64])
    assert tuple(y5[4].shape[-2:]) == (1, 2)
    for i in range(5):
        assert float((y5[i].cpu().to(F64) - r5[i]).abs().max()) <= yardstick_bound(r5[i], T(g12[f"y5_{i}"])), i


# ------------------------------------------------------------------------------------------------------------------ masks, position
def rect_mask(B, H, W, valid):
    m = torch.ones(B, H, W, dtype=torch.bool)
    for b, (h, w) in enumerate(valid):
        m[b, :h, :w] = False
    return m


def mask_cases():
    g = torch.Generator().manual_seed(5)
    rnd = torch.rand(2, 61, 83, generator=g) < 0.4
    rnd[0, :, 50:] = True
    rnd[1, 20:30] = True
    return {
        "R50": (rect_mask(3, 800, 1344, ((800, 1333), (750, 1101), (1, 1))), R50_SIZES),
        "(37, 53) -> (5, 7)": (rect_mask(2, 37, 53, ((37, 53), (20, 31))), ((5, 7),)),
        "random": (rnd, ((31, 42), (16, 21), (8, 11), (61, 83))),
        "fully masked": (torch.ones(2, 40, 64, dtype=torch.bool), ((10, 16), (5, 8))),
        "wider than a workgroup": (rect_mask(2, 24, 600, ((24, 600), (17, 431))), ((12, 300), (24, 600))),    # columns beyond lane 255
    }


def cpu_masks(mask, sizes):
    fm = mask.float()
    masks = [F.interpolate(fm[None], size=hw)[0].to(torch.bool) for hw in sizes]
    return masks, [(~m).int().cumsum(1, dtype=torch.int32) for m in masks], [(~m).int().cumsum(2, dtype=torch.int32) for m in masks]


@pytest.mark.parametrize("name", list(mask_cases()))
def test_masks_and_counts_are_exact(name):
    mask, sizes = mask_cases()[name]
    want = cpu_masks(mask, sizes)
    for m_in in (mask.to(DEV), mask.float().to(DEV) * 3.0):                    # bool, and float with non-zero = padded
        got = neck.pyramid_masks(m_in, sizes)
        for l in range(len(sizes)):
            assert got[0][l].dtype == torch.bool and got[1][l].dtype == torch.int32
            for k in range(3):
                assert torch.equal(got[k][l].cpu(), want[k][l]), (name, l, k)


def pos_reference(ys, xs, dim_t, normalize, scale, eps, offset):
    """float64 sin / cos of the fp32 argument, built on the CPU with the reference's single fp32 operations -> [B, 2F, h, w]."""
    out = []
    for y, x in zip(ys, xs):
        if normalize:
            ye = (y + offset) / (y[:, -1:, :] + eps) * scale
            xe = (x + offset) / (x[:, :, -1:] + eps) * scale
        else:
            ye, xe = y + offset, x + offset
        assert ye.dtype == F32
        ax, ay = (xe.unsqueeze(-1) / dim_t).double(), (ye.unsqueeze(-1) / dim_t).double()
        px = torch.stack((ax.sin(), ax.cos()), -1).flatten(-2)
        py = torch.stack((ay.sin(), ay.cos()), -1).flatten(-2)
        out.append(torch.cat((py, px), 3).permute(0, 3, 1, 2))
    return out


@pytest.mark.parametrize("normalize,offset", [(True, -0.5), (False, 0.0)])
@pytest.mark.parametrize("name,feats", [("R50", 16), ("random", 128), ("fully masked", 16), ("wider than a workgroup", 16)])
def test_position_encoding_at_every_pixel(name, feats, normalize, offset):
    mask, sizes = mask_cases()[name]
    pe = PositionEmbeddingSine(feats, 10000, normalize, offset=offset).to(DEV)
    assert torch.equal(pe.dim_t.cpu(), neck.sine_dim_t(feats, 10000))
    _, ys, xs = cpu_masks(mask, sizes)
    ref = pos_reference(ys, xs, neck.sine_dim_t(feats, 10000), normalize, pe.scale, pe.eps, offset)
    _, gy, gx = neck.pyramid_masks(mask.to(DEV), sizes)
    for dtype in (F32, BF16):
        got = neck.pyramid_sine_pos((gy, gx), pe.dim_t, feats, normalize, pe.scale, pe.eps, offset, dtype)
        for l, hw in enumerate(sizes):
            assert got[l].dtype == dtype and got[l].is_contiguous() and tuple(got[l].shape) == (mask.shape[0], 2 * feats) + tuple(hw)
            err = (got[l].cpu().to(F64) - ref[l]).abs()
            bound = POS_TOL + (2.0 ** -8 * ref[l].abs() if dtype == BF16 else 0.0)
            print(f"pos {name} F {feats} normalize {normalize} {dtype} level {l}: err {float(err.max()):.3e}")
            assert bool((err <= bound).all()), (name, l, dtype, float(err.max()))
    lvl = len(sizes) - 1                                                          # the module on one level mask: the same bits
    m_l = cpu_masks(mask, sizes)[0][lvl].to(DEV)
    assert torch.equal(pe(m_l), neck.pyramid_sine_pos((gy, gx), pe.dim_t, feats, normalize, pe.scale, pe.eps, offset)[lvl])
    assert torch.equal(neck.pyramid_sine_pos([m_l], pe.dim_t, feats, normalize, pe.scale, pe.eps, offset)[0], pe(m_l))


def test_position_encoding_against_g12(g12):
    pe = PositionEmbeddingSine(16, 10000, True, offset=-0.5).to(DEV)
    pe_u = PositionEmbeddingSine(16, 10000, False, offset=0.0).to(DEV)
    builder = PyramidBuilder(golden_mapper(g12, True).to(DEV), pe)
    feats = [T(g12[f"x{i}"]).to(DEV) for i in range(3)]
    with torch.no_grad():
        for img, mk, pk in (("img_mask", "m", "pos"), ("img_mask_rand", "mr", "posr")):
            _, masks, pos = builder(feats, T(g12[img]).to(DEV))
            for i in range(4):
                assert np.array_equal(masks[i].cpu().numpy(), g12[f"{mk}{i}"]), (img, i)
                valid = ~g12[f"{mk}{i}"]
                ok = (valid.any(1, keepdims=True) & valid.any(2, keepdims=True))[:, None]      # exactly the pixels with no last = 0
                got = pos[i].cpu().numpy()
                assert np.isfinite(got).all() and (np.abs(got - g12[f"{pk}{i}"]) * ok).max() <= POS_TOL, (img, i)
        for i in range(4):
            assert np.abs(pe_u(T(g12[f"m{i}"]).to(DEV)).cpu().numpy() - g12[f"posu{i}"]).max() <= POS_TOL, i


# ------------------------------------------------------------------------------------------------------------------ on top
def tiny_model(fused, enc_layers=2, dec_layers=2, num_queries=32):
    from relation_detr_amd import GenerateCDNQueries, RelationCriterion, RelationDETR
    from relation_detr_amd.transformer import build_relation_transformer
    from test_denoising_host import C
    net = build_relation_transformer(num_classes=C, d_ffn=64, enc_layers=enc_layers, dec_layers=dec_layers, num_queries=num_queries,
                                     hybrid_num_proposals=40)
    net.load_state_dict(synthetic_state_dict(net.state_dict()))
    generator = GenerateCDNQueries(num_queries=num_queries, num_classes=C, label_embed_dim=256, denoising_nums=6, fused=True)
    generator.load_state_dict(synthetic_state_dict(generator.state_dict()))
    mapper = ChannelMapper([16, 24, 40], 256, 4, fused=fused)
    mapper.load_state_dict(synthetic_state_dict(mapper.state_dict()))
    pe = PositionEmbeddingSine(128, 10000, True, offset=-0.5, fused=fused)
    return RelationDETR(mapper, pe, net, RelationCriterion(C, fused=True), generator).to(DEV)


def test_pyramid_builder_feeds_the_transformer(g12):
    """Eval detections from the fused pyramid against those from the torch-route pyramid: the fp32 tolerance of tests/test_gpu_parity.py."""
    fused, plain = tiny_model(True).eval(), tiny_model(False).eval()
    feats, mask = [T(g12[f"x{i}"]).to(DEV) for i in range(3)], T(g12["img_mask"]).to(DEV)
    with torch.no_grad():
        pa = PyramidBuilder(fused.neck, fused.position_embedding)(feats, mask)
        pb = PyramidBuilder(plain.neck, plain.position_embedding)(feats, mask)
        for a, b in zip(pa[1], pb[1]):
            assert torch.equal(a, b)
        assert all(p.dtype == F32 and p.is_contiguous() and tuple(p.shape[:2]) == (2, 256) for p in pa[0] + pa[2])
        la, ba = fused(feats, mask)
        lb, bb = plain(feats, mask)
    np.testing.assert_allclose(la.cpu().numpy(), lb.cpu().numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(ba.cpu().numpy(), bb.cpu().numpy(), rtol=0, atol=1e-4)
    with torch.no_grad():                                                         # bf16 position encodings on request
        pos16 = PyramidBuilder(fused.neck, fused.position_embedding)(feats, mask, BF16)[2]
    assert all(p.dtype == BF16 for p in pos16)


def test_pyramid_builder_under_graph_capture(g12):
    model = tiny_model(True).eval()
    builder = PyramidBuilder(model.neck, model.position_embedding)
    feats = [T(g12[f"x{i}"]).to(DEV) for i in range(3)]
    mask = T(g12["img_mask"]).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            for _ in range(2):
                builder(feats, mask)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = builder(feats, mask)
        g = torch.Generator().manual_seed(3)
        for new_mask in (T(g12["img_mask_rand"]), T(g12["img_mask"]).flip(0)):
            for f in feats:
                f.copy_(torch.randn(f.shape, generator=g))
            mask.copy_(new_mask)
            graph.replay()
            eager = builder(feats, mask)
            for a, b in zip(captured[0] + captured[1] + captured[2], eager[0] + eager[1] + eager[2]):
                assert torch.equal(a, b)


def test_train_step_steps_the_neck(g12):
    from relation_detr_amd import denoising as dn
    from relation_detr_amd.optim import FusedAdamW, relation_param_groups, train_step
    from test_denoising_host import C
    z = load_golden("g10_criterion.npz")
    targets = [{"labels": T(z[f"tgt.labels.{b}"]).to(DEV), "boxes": T(z[f"tgt.boxes.{b}"]).to(DEV)} for b in range(2)]
    feats, mask = [T(g12[f"x{i}"]).to(DEV) for i in range(3)], T(g12["img_mask"]).to(DEV)
    noise = dn.cdn_noise(11, 2 * dn.denoising_groups(6, 3) * 5, C, DEV)
    results = {}
    for fused in (True, False):
        model = tiny_model(fused).train()
        before = copy.deepcopy(model.neck.state_dict())
        opt = FusedAdamW(relation_param_groups(model, 1e-3), lr=1e-3, weight_decay=1e-4, fused=True)
        losses, norm = train_step(model, opt, feats, mask, None, targets, max_norm=0.1, noise=noise)
        assert torch.isfinite(norm)
        for k, p in model.neck.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (fused, k)
            assert not torch.equal(p.detach(), before[k]), (fused, k)
        results[fused] = {k: float(v.detach()) for k, v in losses.items()}
    assert set(results[True]) == set(results[False])
    for k, v in results[False].items():
        assert abs(results[True][k] - v) <= 1e-4 * abs(v), (k, results[True][k], v)


def test_outside_the_kernels_conditions_takes_the_torch_route(g12):
    """fp16 autocast, a float64 model and a position module left on the CPU are served by torch, not refused."""
    m = golden_mapper(g12, True).to(DEV)
    xs = [T(g12[f"x{i}"]).to(DEV) for i in range(3)]
    with torch.no_grad():
        want = golden_mapper(g12, False).to(DEV)(xs)
        with torch.autocast("cuda", dtype=torch.float16):
            half = m(xs)
        assert all(float((h.float() - w).abs().max()) <= 2.0 ** -9 * float(w.abs().max()) + 1e-2 for h, w in zip(half, want))
        dbl = m.double()([x.double() for x in xs])
        assert all(d.dtype == F64 and float((d - w.double()).abs().max()) <= 1e-5 for d, w in zip(dbl, want))
        pe = PositionEmbeddingSine(16, 10000, True, offset=-0.5)                   # its table stays on the CPU
        mask = T(g12["m1"]).to(DEV)
        assert torch.equal(pe(mask), copy.deepcopy(pe).to(DEV)(mask))
