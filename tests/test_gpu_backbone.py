"""GPU checks of the ResNet backbone's epilogue kernels (csrc/backbone.hip) and of the modules on top (relation_detr_amd/backbones).

  fp32    bit-equal to torch's own operators in the reference's sequence, evaluated on the same device, forward and backward
  bf16    within 2^-8 |ref| + 2^-20 (|x * s| + |shift| + |res|) of the float64 evaluation on the kernel's own operands: one rounding to
          bf16 plus the fp32 intermediates
Outputs are allocated under tests/dirty.py's poison, so an element a kernel does not write shows as NaN or 48.5.  The shapes are the
smallest that reach each path: one element, planes off the 16-byte grid, planes shorter than a piece, several pieces, several chunks
of a plane, channels-last with C below, equal to, above and no multiple of the piece."""
import copy
import itertools

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import relation_detr_amd
from dirty import poisoned
from helpers import bf16_slack, torch_bn_act, torch_stem
from relation_detr_amd import backbones
from relation_detr_amd.backbones import FrozenBatchNorm2d, ResNetBackbone, frozen_bn_act, frozen_bn_act_backward, stem_bn_relu_maxpool

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
NCHW_SHAPES = [(1, 1, 1, 1), (2, 3, 7, 9), (1, 5, 1, 17), (2, 64, 5, 8), (3, 256, 13, 21)]
NHWC_SHAPES = [(2, c, 5, 7) for c in (3, 64, 72, 260)]
LAYOUTS = [(s, False) for s in NCHW_SHAPES] + [(s, True) for s in NHWC_SHAPES]
POOL_SIZES = [(1, 1), (2, 2), (7, 9), (8, 8), (15, 22), (9, 24)]        # W = 8 and 24: the NCHW rows kernel, one and three lanes a row


def ident(case):
    shape, cl = case
    return ("nhwc" if cl else "nchw") + "x".join(str(s) for s in shape)


def make(shape, cl, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if cl else t


def constants(C, seed):
    g = torch.Generator().manual_seed(seed)
    s = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    return s.to(DEV), (torch.randn(C, generator=g) * 0.5).to(DEV)


def same(a, b):
    """Equal element by element, a NaN equal to a NaN."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (a.isnan() & b.isnan())).all())


def check_forward(got, x, s, h, r, relu, dtype, what):
    assert got.dtype == dtype and got.shape == x.shape, what
    if dtype == F32:
        assert torch.equal(got, torch_bn_act(x, s, h, r, relu)), what
    else:
        ref = torch_bn_act(x.double(), s.double(), h.double(), None if r is None else r.double(), relu)
        err = (got.double() - ref).abs()
        assert bool((err <= 2.0 ** -8 * ref.abs() + bf16_slack(x, s, h, r)).all()), (what, float(err.max()))


# ------------------------------------------------------------------------------------------------------------- frozen_bn_act
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", LAYOUTS, ids=ident)
def test_frozen_bn_act_forward(case, dtype):
    shape, cl = case
    x, r = make(shape, cl, dtype, 1), make(shape, cl, dtype, 2)
    s, h = constants(shape[1], 3)
    for with_r, relu, byte in itertools.product((False, True), (False, True), (0xFF, 0x42)):
        res = r if with_r else None
        what = (shape, cl, with_r, relu, byte)
        with poisoned(byte) as p:
            got = frozen_bn_act(x, s, h, residual=res, relu=relu)
            assert p.fills >= 1
        assert got.data_ptr() != x.data_ptr() and got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        check_forward(got, x, s, h, res, relu, dtype, what)
        work = x.clone(memory_format=torch.preserve_format)
        back = frozen_bn_act(work, s, h, residual=res, relu=relu, out=work)
        assert back.data_ptr() == work.data_ptr() and torch.equal(back, got), what      # in place: the same values
        with poisoned(byte):
            out = torch.empty_like(x)
        assert frozen_bn_act(x, s, h, residual=res, relu=relu, out=out) is out and torch.equal(out, got), what


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
def test_frozen_bn_act_keeps_nan_and_infinities(cl):
    shape = (2, 6, 5, 7)
    x, r = make(shape, cl, F32, 4), make(shape, cl, F32, 5)
    s, h = constants(6, 6)
    flat = x.view(-1) if not cl else x.permute(0, 2, 3, 1).reshape(-1)
    flat[3], flat[50], flat[97], flat[200], flat[333] = float("nan"), float("inf"), float("-inf"), float("nan"), float("inf")
    for with_r, relu in itertools.product((False, True), (False, True)):
        res = r if with_r else None
        got, want = frozen_bn_act(x, s, h, residual=res, relu=relu), torch_bn_act(x, s, h, res, relu)
        assert bool(want.isnan().any()) and bool(want.isinf().any()) and same(got, want), (with_r, relu)
        got16 = frozen_bn_act(x.to(BF16), s, h, residual=None if res is None else res.to(BF16), relu=relu)
        assert torch.equal(got16.isnan(), want.isnan()), (with_r, relu)


def test_frozen_bn_act_copies_what_is_not_dense_and_converts_the_residual():
    s, h = constants(8, 7)
    big = make((2, 8, 9, 12), False, F32, 8)
    crop, r = big[:, :, 1:8, 2:11], make((2, 8, 7, 9), True, BF16, 9)              # a crop; a residual of the other layout and dtype
    got = frozen_bn_act(crop, s, h, residual=r)
    assert torch.equal(got, torch_bn_act(crop, s, h, r.float(), True)) and got.is_contiguous()
    with pytest.raises(ValueError):
        frozen_bn_act(crop, s, h, out=crop)
    with pytest.raises(ValueError):
        frozen_bn_act(big, s.double(), h)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", LAYOUTS, ids=ident)
def test_frozen_bn_act_backward(case, dtype):
    shape, cl = case
    s, h = constants(shape[1], 11)
    gy = make(shape, cl, dtype, 12)
    for with_r, relu, in_place in itertools.product((False, True), (False, True), (False, True)):
        what = (shape, cl, with_r, relu, in_place)
        x = make(shape, cl, dtype, 13).requires_grad_()
        r = make(shape, cl, dtype, 14).requires_grad_() if with_r else None
        with poisoned(0xFF):
            if in_place:
                work = x.clone(memory_format=torch.preserve_format)
                y = frozen_bn_act(work, s, h, residual=r, relu=relu, out=work)
                assert y.data_ptr() == work.data_ptr()
            else:
                y = frozen_bn_act(x, s, h, residual=r, relu=relu)
            y.backward(gy)
        if dtype == F32:
            x2 = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
            r2 = r.detach().clone(memory_format=torch.preserve_format).requires_grad_() if with_r else None
            torch_bn_act(x2, s, h, r2, relu).backward(gy)
            assert torch.equal(x.grad, x2.grad), what
            assert r is None or torch.equal(r.grad, r2.grad), what
        else:
            masked = gy.double() * (~(y.detach() <= 0)).double() if relu else gy.double()       # on the kernel's own output
            ref = masked * s.double().reshape(1, -1, 1, 1)
            assert x.grad.dtype == BF16 and bool(((x.grad.double() - ref).abs() <= 2.0 ** -8 * ref.abs()).all()), what
            assert r is None or torch.equal(r.grad.double(), masked), what
        # the kernel call alone: dres only when asked for
        dx, dres = frozen_bn_act_backward(gy, y.detach(), s, relu, want_dres=False)
        assert dres is None and torch.equal(dx, x.grad), what
        with poisoned(0x42):
            dx, dres = frozen_bn_act_backward(gy, y.detach() if relu else None, s, relu, want_dres=True)
        assert torch.equal(dx, x.grad) and (r is None or torch.equal(dres, r.grad)), what


def test_residual_without_a_gradient_gets_none():
    s, h = constants(5, 15)
    x, r = make((1, 5, 3, 4), False, F32, 16).requires_grad_(), make((1, 5, 3, 4), False, F32, 17)
    frozen_bn_act(x, s, h, residual=r).sum().backward()
    assert r.grad is None and x.grad is not None


# ------------------------------------------------------------------------------------------------------------- stem_pool
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
def test_stem_pool(cl, dtype):
    for (H, W), C, byte in itertools.product(POOL_SIZES, (1, 3, 64), (0xFF, 0x42)):
        x = make((2, C, H, W), cl, dtype, 20 + H + C)
        s, h = constants(C, 21)
        with poisoned(byte):
            got = stem_bn_relu_maxpool(x, s, h)
        what = (H, W, C, cl, byte)
        assert tuple(got.shape) == (2, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1) and got.dtype == dtype, what
        assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format), what
        if dtype == F32:
            assert torch.equal(got, torch_stem(x, s, h)), what
        else:
            ref = torch_stem(x.double(), s.double(), h.double())
            slack = F.max_pool2d(bf16_slack(x, s, h, None), 3, 2, 1)
            assert bool(((got.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + slack).all()), what


@pytest.mark.parametrize("W", [9, 16])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
def test_stem_pool_negative_windows_and_nan(cl, W):
    x = -make((2, 8, 7, W), cl, F32, 30).abs() - 0.5
    s, h = torch.rand(8, device=DEV) + 0.5, -torch.rand(8, device=DEV)
    got = stem_bn_relu_maxpool(x, s, h)
    assert not got.view(torch.int32).any()                                          # every window all negative: +0, never the padding
    x = make((2, 8, 7, W), cl, F32, 31)
    x[1, 3, 3, 5], x[0, 0, 0, 0] = float("nan"), float("nan")
    s, h = constants(8, 32)
    got, want = stem_bn_relu_maxpool(x, s, h), torch_stem(x, s, h)
    assert int(got.isnan().sum()) == 4 + 1 and same(got, want)                      # (3, 5) lies in four windows, the corner in one
    with pytest.raises(relation_detr_amd._lib.RdetrError):
        stem_bn_relu_maxpool(x.requires_grad_(), s, h)


# ------------------------------------------------------------------------------------------------------------- the network
def randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=g) * 1.5 + 0.25)
            elif name.endswith("running_mean"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.3)
            elif name.endswith("bias"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.2)
            elif t.dim() == 1:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            else:
                t.copy_(torch.randn(t.shape, generator=g) * (1.5 / t[0].numel()) ** 0.5)
    return model


def ulps_of_max(got, ref):
    """max |got - ref| in units of the fp32 spacing at the reference's largest magnitude."""
    ref = ref.detach().double().cpu().numpy()
    return float(np.abs(got.detach().double().cpu().numpy() - ref).max() / np.spacing(np.float32(np.abs(ref).max())))


class deterministic_convolutions:
    """The library's convolutions may add with atomics; the two routes hand them identical operands, and equal results need them to
    do the same thing twice (tests/test_gpu_images.py does the same for the neck's extra level)."""

    def __enter__(self):
        self.was = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.was


def both_routes(model, x):
    assert model.fused and model.takes_fused_route(x)
    with torch.no_grad(), deterministic_convolutions():
        fused = model(x)
        model.fused = False
        assert not model.takes_fused_route(x)
        plain = model(x)
        model.fused = True
    return fused, plain


@pytest.fixture(scope="module")
def r50():
    return randomise(ResNetBackbone("resnet50", return_indices=(1, 2, 3), freeze_indices=(0,)), 40).to(DEV).eval()


@pytest.fixture(scope="module")
def image():
    return torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(41)).to(DEV)


@pytest.mark.parametrize("arch", ["resnet50", "resnet18", "resnext50_32x4d", "resnet50-channels-last"])
def test_network_fused_route_equals_the_torch_route_fp32(arch, r50, image):
    channels_last = arch.endswith("-channels-last")
    arch = arch.split("-")[0]
    model = r50 if arch == "resnet50" else randomise(ResNetBackbone(arch, return_indices=(1, 2, 3), freeze_indices=(0,)), 42).to(DEV).eval()
    x = image.contiguous(memory_format=torch.channels_last) if channels_last else image
    fused, plain = both_routes(model, x)
    assert list(fused) == ["layer2", "layer3", "layer4"] == list(plain)
    for k, c in zip(fused, model.num_channels):
        assert tuple(fused[k].shape[:2]) == (2, c) and fused[k].is_contiguous() and fused[k].dtype == F32
        worst = ulps_of_max(fused[k], plain[k])
        print(f"{arch}{' channels-last' if channels_last else ''} {k}: fused vs torch route {worst:.2f} ulp of the maximum")
        assert worst <= 4.0, (k, worst)


def test_training_step_gradients_match_the_torch_route(r50, image):
    model = copy.deepcopy(r50).train()
    gs = None

    def grads(fused):
        nonlocal gs
        model.fused = fused
        model.zero_grad(set_to_none=True)
        out = model(image)
        if gs is None:
            gen = torch.Generator().manual_seed(43)
            gs = {k: torch.randn(v.shape, generator=gen).to(DEV) for k, v in out.items()}
        sum((out[k] * gs[k]).sum() for k in out).backward()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}

    with deterministic_convolutions():
        fused, plain, again = grads(True), grads(False), grads(False)
    worst = 0.0
    for n, p in model.named_parameters():
        if not p.requires_grad:
            assert n.split(".")[0] in ("conv1", "layer1") and fused[n] is None and plain[n] is None, n
            continue
        spacing = float(np.spacing(np.float32(plain[n].abs().max().item())))
        own = float((plain[n] - again[n]).abs().max())                              # the torch route against itself
        err = float((fused[n] - plain[n]).abs().max())
        worst = max(worst, err / spacing)
        assert err <= max(4.0 * spacing, 2.0 * own), (n, err / spacing, own / spacing)
    assert sum(p.requires_grad for p in model.parameters()) == 42                   # 53 convolutions less the stem's and layer1's ten
    print(f"resnet50 training step: worst parameter gradient {worst:.2f} ulp of its maximum from the torch route")


def test_network_bf16_rounds_less_often_than_the_torch_route(r50, image):
    with torch.no_grad(), deterministic_convolutions():
        want = ResNetBackbone.forward_torch(r50, image)
    model = copy.deepcopy(r50).to(BF16)
    fused, plain = both_routes(model, image.to(BF16))

    def rel_l2(got):
        num = sum(float((got[k].double() - want[k].double()).pow(2).sum()) for k in want)
        return (num / sum(float(want[k].double().pow(2).sum()) for k in want)) ** 0.5

    e_fused, e_plain = rel_l2(fused), rel_l2(plain)
    print(f"resnet50 bf16, relative L2 error against the fp32 torch route: fused {e_fused:.4e}, torch route {e_plain:.4e}")
    assert all(v.dtype == BF16 for v in fused.values())
    assert e_fused <= 1.25 * e_plain, (e_fused, e_plain)


def test_autocast_keeps_the_convolutions_bf16(r50, image):
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        assert r50.takes_fused_route(image)
        out = r50(image)
    assert all(v.dtype == BF16 and bool(torch.isfinite(v).all()) for v in out.values())
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert not r50.takes_fused_route(image)


def test_graph_capture_replays_the_eager_forward(image):
    model = randomise(ResNetBackbone("resnet18", return_indices=(1, 2, 3), freeze_indices=(0,)), 44).to(DEV).eval()
    static = image.clone()
    with torch.no_grad(), deterministic_convolutions():
        eager = model(static)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(static)                                                           # warm-up: the library's plans, the cached constants
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = model(static)
        static.copy_(image.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        flipped = model(image.flip(0))
    for k in eager:
        assert torch.equal(captured[k], flipped[k]) and not torch.equal(captured[k], eager[k]), k


# ------------------------------------------------------------------------------------------------------------- the detector
def test_detector_with_the_r50_backbone_end_to_end():
    torch.manual_seed(45)
    C = 11
    model = relation_detr_amd.relation_detr_r50(num_classes=C, num_queries=30, hybrid_num_proposals=30, enc_layers=2, dec_layers=2, d_ffn=64,
                                                denoising_nums=6, min_size=64, max_size=100, num_select=10)
    randomise(model.backbone, 46)
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(47)
    images = [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g).to(DEV) for h, w in ((70, 100), (96, 71))]
    with torch.no_grad(), deterministic_convolutions():
        dets, tensor = model(images)
        model.backbone.fused = False
        dets_plain, tensor_plain = model(images)
        model.backbone.fused = True
    assert tuple(tensor.shape) == (2, 10, 6) and bool(torch.isfinite(tensor).all()) and len(dets) == 2
    for d in dets:
        assert set(d) == {"scores", "labels", "boxes"} and tuple(d["boxes"].shape) == (10, 4) and d["labels"].dtype == torch.int64
    assert torch.equal(tensor, tensor_plain)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(dets, dets_plain) for k in a)

    model.train()
    floats = [torch.randn(3, h, w, generator=g).to(DEV) for h, w in ((64, 96), (70, 57))]
    targets = [{"labels": torch.tensor([1, 7, 3], device=DEV), "boxes": torch.tensor([[4.0, 6.0, 40.0, 50.0], [10.0, 2.0, 90.0, 30.0],
                                                                                      [50.0, 20.0, 70.0, 60.0]], device=DEV)},
               {"labels": torch.tensor([0, 10], device=DEV), "boxes": torch.tensor([[5.0, 5.0, 30.0, 60.0], [20.0, 10.0, 50.0, 40.0]], device=DEV)}]
    losses = model(floats, targets)
    suffixes = ("", "_0", "_enc", "_dn", "_dn_0", "_hybrid", "_0_hybrid", "_enc_hybrid")      # two decoder layers: one auxiliary output
    expected = {f"loss_{n}{s}" for n in ("class", "bbox", "giou") for s in suffixes}
    assert set(losses) == expected, set(losses) ^ expected
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    assert model.backbone.layer2[0].conv1.weight.grad is not None and model.backbone.layer1[0].conv1.weight.grad is None
    assert bool(torch.isfinite(model.backbone.layer4[2].conv3.weight.grad).all())
